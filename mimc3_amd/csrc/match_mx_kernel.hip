// match_mx_kernel.hip -- DLC/NCC matcher for gfx950 on the matrix cores: 8-bit imagery, DENSE correlation surfaces.
//
// Same contract as match_px_kernel.hip (matching_ncc_dlc_2, MIMC_module.c:805-842), for the points whose reachable cell grid
// fits one 32 x 32 tile.  One workgroup of two wave64 = one grid point (wave w owns the cell columns [16 w, 16 w + 16)).  Instead of
// evaluating the cells a hill climb asks for (a request queue, evaluation batches, a speculative climb that waits for them), the
// kernel builds the COMPLETE surface of the tile:
//
//   sxy[dy][s] = sum_r sum_k a[r][k] * b[r + dy][k + s]                              (MIMC_module.c:719-733, the product stream)
//              = sum_r (W_r T_r)[dy][s]     W_r[dy][j] = b[r + dy][j]   A operand: 16 window rows, plain 16-byte LDS reads
//                                           T_r[j][s]  = a[r][j - s]    B operand: the Toeplitz band of chip row r, 0 outside
//   i.e. per chip row, 64 window columns and 16 x 16 cells one v_mfma_i32_16x16x64_i8, all into the cells' i32 accumulators (exact
//   integers).  u8 -> i8:  a' = a - 128 (a ^ 0x80), b' = b - 128, Toeplitz padding a' = 0:
//              sum ab = sum a'b' + 128 sum_box b + 128 sum a - 128^2 CW^2        (a null is a zero factor: no mask anywhere)
//   * window-side sums  sy = sum_box b, syy = sum_box b^2  of every cell: row-box sums by MFMA against a band of ones
//     (b^2 as two byte planes), then the vertical CW-row sums by a second MFMA against a band of ones (the row sums split
//     into byte planes; an accumulator tile is the next MFMA's B operand as it stands: its rows are the K index) -- the record
//     forms (RecCfg) read them from the window plane's packed table instead, for the cells they will finish (BOXT below);
//   * null pixels (the two forms for null-ridden points, built and tested but not taken by default: launch_match_mx has the
//     measurements).  A window null q of the box takes a(q) out of n, sx, sxx: with zb = [b == 0] as the A operand the corrections
//     are three more correlations on the same pipe -- sum zb (box count), sum a zb (same B operand as sxy), sum a^2 zb (a^2 as two
//     byte planes of the chip) -- the window-null form.  A chip null p takes b(p) out of sy, syy: with za = [a == 0] as the B operand
//     -- formed from the Toeplitz rows of the chip rows that hold nulls, the only ones visited -- sum b za, sum b^2 za (b^2 as two
//     byte planes of the A operand), and sum zb za for n -- the general form.  The never-written last window row / column (T4) are
//     zeros of the staged tile, i.e. nulls like any other when the window's nulls are correlated anyway; in the clean form they are
//     applied in closed form: they take the chip's last column / row out of n, sx, sxx (table queries of the chip plane);
//   * the NCC of all 1,024 cells (:734, f64, no contraction; a guarded fast reciprocal square root with the exact sqrt / division
//     for the cells within 2^13 f64 ulps of an f32 rounding boundary) -> one f32 surface in LDS;
//   * the climb of every pivot on the complete surface (lane k = pivot k), the exact replay of the reference's sequential
//     visited-set semantics (:691-753) and the 3x3 fit (:757-788) as in match_px_kernel.hip -- on wave 0, wave 1 has left by then.
// What this kernel does not take goes to the register-tiled kernel (match_px_kernel.hip) without a host round trip.  A point with nulls
// in its window or chip, more than 64 pivots or a pivot set wider than the tile is known from table queries before any kernel runs:
// u8_classify (u8_classify_kernel.hip, one thread per point, once per call) writes the class byte of every point and two index lists
// in ascending point order, and this kernel's DLC launch runs over the clean list only -- a point it does not take never issues a
// tile or chip load.  A climb that leaves the tile or outlasts the 16 recorded scans (a few dozen points per launch) is only known
// here: such a point is appended to the rest list with one atomicAdd, and the register-tiled kernel runs over that list right behind.
// With point records (U8PointRec, match_kernel.h; RecCfg below) the classifier also leaves, at every list position, the header it has read
// and derived of that point: the clean form starts from that one record, and a point it appends takes its record along.
// Behind its clean list the same launch tries the advance list: window-null points whose climb area holds no null, for which the clean
// form's cells inside that area are exact (mx_climb_area, match_kernel.h) -- finished only if every scan stays inside it.
// Clean points carry their climb area as well (MIMC3_MX_AREA=0: the whole tile): the accumulator rows are banded (band_row below), one
// iteration of the NCC finish is four consecutive tile rows, and the RecCfg form finishes only the bands that meet the area -- a clean
// point whose climb leaves its area goes to the rest list as one whose climb leaves the tile does.
// (The exhaustive search classifies in the clean form's header and hands on through the class byte alone: every one of its points
// stays on this kernel's forms, which run behind in flag mode.)
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include "match_kernel.h"
#include "sat_kernel.h"
#include "match_full_tail.h"

namespace mimc3 {

namespace mx {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t alignb(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_alignbyte(hi, lo, s); }
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
// a wave-uniform value the compiler loaded through the vector memory path (global stores in the kernel keep it from using scalar loads): into SGPRs
__device__ __forceinline__ unsigned long long uni64(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ v4i mfma(const v4i &a, const v4i &b, const v4i &c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }


template <int OCW_, bool GEN_, bool CN_ = GEN_>
struct Cfg {
    static constexpr int OCW = OCW_, CW = 2 * OCW_ + 1, NPX = CW * CW;
    static constexpr bool GEN = GEN_;                   // null pixels in the window ...
    static constexpr bool CN = CN_;                     // ... and in the chip (false with GEN: the window-null form -- half the accumulators, a wave more per SIMD)
    // Two waves per grid point: wave w owns the cell columns [16 w, 16 w + 16) of the 32 x 32 tile (two 16 x 16 MFMA tiles, rows
    // 0..15 and 16..31), so each wave carries half the accumulators.  The front phases run on both, the climb / replay / fit on wave 0
    // after wave 1 has left: registers per wave, not LDS, bound how many points a CU works on.
    static constexpr int NW = 2, NT = 64 * NW;
    static constexpr int KW = CW + 31;                  // window columns (and rows) the 32 x 32 cells of a tile reach
    static constexpr int KCW = (CW + 15 + 63) / 64;     // MFMAs per chip row and 16 x 16 cell tile (K chunks of 64 window columns, from column 16 w)
    static constexpr int RDW = 16 * (NW - 1) + 64 * KCW;   // bytes of a tile row some wave reads
    static constexpr int SW = (KW + 15) & ~15;          // bytes of a tile row that are staged (what lies beyond is only ever weighted 0)
    static constexpr int PW0 = RDW > SW ? RDW : SW;
    static constexpr int PW = ((PW0 / 16) & 1) ? PW0 : PW0 + 16;   // pitch 16 x odd: few bank conflicts between the rows of a ds_read_b128 group
    static constexpr int NTR = (KW + 15) / 16;          // 16-row tiles of the row-box sums
    static constexpr int KCV = (NTR + 3) / 4;           // K chunks (64 tile rows) of the vertical sums
    static constexpr int CD = (CW + 3) / 4;             // dwords per chip row
    static constexpr int LASTN = CW - 4 * (CD - 1);     // valid bytes of a chip row's last dword
    static constexpr int CP0 = (CW + 15 + 3) & ~3;
    static constexpr int CP = CP0 > 64 * KCW ? CP0 : 64 * KCW;     // chip plane pitch: a row's right padding is the next row's left padding
    static constexpr int CH0 = 16;                      // leading zeros (row 0's left padding)
    static constexpr int CWE = CW + (CW & 1);           // chip rows the product loop walks: two per trip (an all-zero row behind an odd chip)
    static constexpr int CHB = (CH0 + CWE * CP + 16 + 15) & ~15;   // one chip plane (+ the read-ahead of the last row's last lane)
    static constexpr int VP = 33;                       // pitch (words) of the NCC surface
    static constexpr int LDS_W = (16 * NTR + 1) * PW;   // (+ the row the product loop's zero chip row reads)
    static constexpr int LDS_VAL = 4 * 32 * VP;
    static constexpr int NPL = GEN_ ? 3 : 1;            // chip planes: a', and in the general form (a^2 & 255)', (a^2 >> 8)' (the B operands of the window-null corrections)
    // general form, small chips: the window's null plane (0x80 where b == 0) staged next to the tile, so that the A operand of the window-null
    // correlations is a load; the big chips, short of LDS, form it from the tile's bytes in registers (3 instructions per dword)
    static constexpr bool ZPL = GEN_ && OCW_ <= 16;
    static constexpr int OFF_Z = ((LDS_W > LDS_VAL ? LDS_W : LDS_VAL) + 15) & ~15;       // the surface reuses the tile's bytes once the sums are in registers
    static constexpr int OFF_CH = OFF_Z + (ZPL ? LDS_W : 0);
    static constexpr int OFF_VIS = OFF_CH + NPL * CHB;
    static constexpr int OFF_PIV = OFF_VIS + 128;      // the pivots' starts, parked for wave 0's climbs
    static constexpr int OFF_RM = OFF_PIV + 512;       // general form: bit r = chip row r holds a null pixel
    static constexpr int LDS = OFF_RM + 16;
    static constexpr int WGS = 163840 / ((LDS + 255) & ~255);      // workgroups per CU that LDS admits
    static constexpr int MINW0 = GEN_ ? (CN_ ? 3 : 4) : 8;          // occupancy target, waves per SIMD (register budget) ...
    static constexpr int MINW1 = (WGS * NW) / 4 > 0 ? (WGS * NW) / 4 : 1;                   // ... never above what LDS admits anyway
    static constexpr int MINW = MINW0 < MINW1 ? MINW0 : MINW1;
    static constexpr bool FULL = false;                 // the DLC matcher (true: FullCfg, the exhaustive search)
    static constexpr bool PEAK = false;                 // full mode: also write the arg-max cell to full_peak (FullPeakCfg)
    static constexpr bool MULTI = false;                // full mode: also write the best local maxima as candidates to full_cand (FullMultiCfg)
    static constexpr bool SURF = false;                 // full mode: also store the finished surface to full_surf (FullSurfCfg, FullMultiSurfCfg)
    static constexpr bool REC = false;                  // the header comes from u8_classify's point record (RecCfg)
    static constexpr bool BOXT = false;                 // the window-side box sums come from the window plane's packed table (RecCfg), not from MFMAs
};
// The clean form behind u8_classify with point records (U8PointRec, match_kernel.h): workgroup b starts from the record at list position b
// -- one load behind the list length -- instead of the list entry, the point row and pivot range, the last pivot and the table queries,
// each of which waited for the one before.  Everything behind the header is Cfg<OCW_, false>'s
// BOXT_: sum_box b and sum_box b^2 of the cells the finish will run are read from the window plane's packed table (sat_kernel.h: four
// entries per cell, the T4 column and row by a clamp of the far corner -- sat_cell_corners) instead of being recomputed for all 1,024
// cells by MFMAs against bands of ones; false (MIMC3_MX_BOX_TABLE=0): the MFMA box sums, as in every other form
template <int OCW_, bool BOXT_ = true>
struct RecCfg : Cfg<OCW_, false, false> {
    static constexpr bool REC = true;
    static constexpr bool BOXT = BOXT_;
};
// Exhaustive search (mimc3_match_ncc_full): the same surface builder on the cell tile whose origin is c - R (the search centre
// c = uv0 + offset + shift, 1 <= R <= 15: all (2R + 1)^2 cells in the tile), no never-written row / column (T4), and instead of the
// climb, replay and fit the first-wins arg-max, the border / validity rule, the reference's fit, the SNR and the fit's Hessian
template <int OCW_, bool GEN_, bool CN_>
struct FullCfg : Cfg<OCW_, GEN_, CN_> {
    static constexpr bool FULL = true;
};
// ... and for a level of the coarse-to-fine search (mimc3_match_ncc_pyramid): the same record, plus every point's arg-max cell k (or -1)
// in full_peak, where the next level's search centre comes from
template <int OCW_, bool GEN_, bool CN_>
struct FullPeakCfg : FullCfg<OCW_, GEN_, CN_> {
    static constexpr bool PEAK = true;
};

// ... and with candidates (mimc3_match_ncc_full_multi): the same record, plus the best full_npeaks local maxima of the surface as
// (du, dv, ncc) candidates in full_cand, pass-major -- what mimc3_cluster_candidates reads as dp
template <int OCW_, bool GEN_, bool CN_>
struct FullMultiCfg : FullCfg<OCW_, GEN_, CN_> {
    static constexpr bool MULTI = true;
};

// ... and with the surfaces (mimc3_match_ncc_full_surf, the stack's class layers): the record-only form and the form with candidates,
// each also storing the point's finished f32 surface to full_surf in k order; all NaN where the point leaves before it has one.  Only
// the form that finishes a point stores it: the clean form hands null-ridden points on, the flag-mode forms behind it store theirs.
// (Template forms and not a run-time branch: the kernel is register-tight, and the existing instantiations keep their code.)
template <int OCW_, bool GEN_, bool CN_>
struct FullSurfCfg : FullCfg<OCW_, GEN_, CN_> {
    static constexpr bool SURF = true;
};
template <int OCW_, bool GEN_, bool CN_>
struct FullMultiSurfCfg : FullMultiCfg<OCW_, GEN_, CN_> {
    static constexpr bool SURF = true;
};

// The constant band operands, one table per chip size (constant-initialised device data).  v_mfma_i32_16x16x64_i8: lane (n = lane & 15,
// h = lane >> 4) holds byte i of K slot (h, i) of row / column n.
//   bm[c][lane]     : 0xff in the bytes of a chip-row B operand that hold chip pixels (the others are Toeplitz padding) -- the same bytes as hb
//   hb[c][lane]     : B operand of the row-box sums -- byte i of chunk c <-> window column x = 16 w + 64 c + 16 h + i, cell column
//                     s = 16 w + n:  1 if s <= x < s + CW  (the wave index cancels)
//   vb[m][c][lane]  : A operand of the vertical sums -- cell row dy = 16 m + band_row(n), the banded row order of the product
//                     accumulators (band_row below); K slot (h, i) of chunk c <-> tile row
//                     y = 64 c + 16 (i >> 2) + 4 (i & 3) + h, where the accumulator layout of the row sums puts it (register i & 3 of row
//                     tile 4 c + (i >> 2); the row sums read their A operand through the products' banded rows):  1 if dy <= y < dy + CW
// Banded accumulator rows: MFMA row j of a 16 x 16 cell tile holds tile row 4 (j & 3) + (j >> 2), so that register i of lane (n, h) --
// MFMA row 4 h + i -- is tile row 4 i + h: the four lane groups of register i cover the four CONSECUTIVE rows 4 i .. 4 i + 3, and one
// iteration of the NCC finish is one band of four rows, which a whole wave can skip.  The A operand of the products and the ones-band
// of the vertical box sums put their rows in this order; the surfaces in LDS stay in natural order
constexpr int band_row(int j) { return 4 * (j & 3) + (j >> 2); }
template <int CW, int KCW, int KCV>
struct alignas(16) Bands {
    uint32_t hb[KCW][64][4], vb[2][KCV][64][4], bm[KCW][64][4];
    constexpr Bands() : hb(), vb(), bm()
    {
        for (int l = 0; l < 64; l++) {
            const int n = l & 15, h = l >> 4;
            for (int i = 0; i < 16; i++) {
                for (int c = 0; c < KCW; c++) {
                    const int x = 64 * c + 16 * h + i;
                    if (n <= x && x < n + CW) { hb[c][l][i >> 2] |= 1u << (8 * (i & 3)); bm[c][l][i >> 2] |= 0xffu << (8 * (i & 3)); }
                }
                for (int m = 0; m < 2; m++)
                    for (int c = 0; c < KCV; c++) {
                        const int dy = 16 * m + band_row(n), y = 64 * c + 16 * (i >> 2) + 4 * (i & 3) + h;
                        if (dy <= y && y < dy + CW) vb[m][c][l][i >> 2] |= 1u << (8 * (i & 3));
                    }
            }
        }
    }
};
template <int CW, int KCW, int KCV> __device__ const Bands<CW, KCW, KCV> kBands{};

constexpr int kStatW = 9;        // (slot 7: advance list, slot 8: replay-shortcut outcome + 1)

// u8 pixels back from the signed bytes of an A operand, squared, split into the byte planes (x^2 & 255) and (x^2 >> 8), as signed bytes
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
// the squares of the four pixels of a dword as the two byte planes (x^2 & 255, x^2 >> 8): the bytes spread to 16-bit halves (v_perm),
// two packed 16-bit multiplies (a byte's square fits 16 bits), the planes picked out by v_perm -- 6 instructions
__device__ __forceinline__ void squares_dword(uint32_t x, uint32_t &lo, uint32_t &hi)
{
    const uint32_t u01 = perm(0u, x, 0x0c010c00u), u23 = perm(0u, x, 0x0c030c02u);           // [b0, 0, b1, 0], [b2, 0, b3, 0]  (selector 0x0c: the byte 0)
    const us2 p01 = __builtin_bit_cast(us2, u01), p23 = __builtin_bit_cast(us2, u23);
    const uint32_t q01 = __builtin_bit_cast(uint32_t, (us2)(p01 * p01)), q23 = __builtin_bit_cast(uint32_t, (us2)(p23 * p23));
    lo = perm(q23, q01, 0x06040200u);
    hi = perm(q23, q01, 0x07050301u);
}
__device__ __forceinline__ void squares(const v4i &a, v4i &lo, v4i &hi)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t l, g;
        squares_dword((uint32_t)a[k] ^ 0x80808080u, l, g);
        lo[k] = (int)(l ^ 0x80808080u); hi[k] = (int)(g ^ 0x80808080u);
    }
}
// 0x80 (the signed byte -128) in every byte of an operand that is a null pixel (its signed byte is 0x80, i.e. the pixel 0; Toeplitz padding
// is 0x00): three instructions per dword.  A correlation with this plane is -128 times the correlation with the 0 / 1 null mask -- exactly
__device__ __forceinline__ uint32_t null80(uint32_t x) { return x & ~((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u; }
__device__ __forceinline__ v4i null80v(const v4i &a)
{
    v4i z;
#pragma unroll
    for (int k = 0; k < 4; k++) z[k] = (int)null80((uint32_t)a[k]);
    return z;
}
// 1 in every byte of the A operand that is a null pixel (b == 0, i.e. b' == 0x80)
__device__ __forceinline__ v4i nullbytes(const v4i &a)
{
    v4i z;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t x = (uint32_t)a[k] ^ 0x80808080u;
        const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;           // 0x80 in every non-zero byte
        z[k] = (int)((nz ^ 0x80808080u) >> 7);
    }
    return z;
}
// The four registers of a 16 x 16 accumulator tile (rows 4 h + 0..3 of one 16-row tile) as ONE dword of each byte plane of the next
// MFMA's B operand (signed bytes: ^ 0x80, except the single plane of values < 128)
__device__ __forceinline__ void planes2(const v4i &R, uint32_t &p0, uint32_t &p1)
{
    const uint32_t t01 = perm((uint32_t)R[1], (uint32_t)R[0], 0x05010400u), t23 = perm((uint32_t)R[3], (uint32_t)R[2], 0x05010400u);   // [r0.b0, r1.b0, r0.b1, r1.b1]
    p0 = perm(t23, t01, 0x05040100u) ^ 0x80808080u;
    p1 = perm(t23, t01, 0x07060302u) ^ 0x80808080u;
}
__device__ __forceinline__ void planes3(const v4i &R, uint32_t &p0, uint32_t &p1, uint32_t &p2)
{
    const uint32_t r0 = (uint32_t)R[0], r1 = (uint32_t)R[1], r2 = (uint32_t)R[2], r3 = (uint32_t)R[3];
    const uint32_t t01 = perm(r1, r0, 0x05010400u), t23 = perm(r3, r2, 0x05010400u);
    const uint32_t u01 = perm(r1, r0, 0x07030602u), u23 = perm(r3, r2, 0x07030602u);     // [r0.b2, r1.b2, r0.b3, r1.b3]
    p0 = perm(t23, t01, 0x05040100u) ^ 0x80808080u;
    p1 = perm(t23, t01, 0x07060302u) ^ 0x80808080u;
    p2 = perm(u23, u01, 0x05040100u) ^ 0x80808080u;
}
__device__ __forceinline__ uint32_t planes1(const v4i &R)
{
    const uint32_t t01 = perm((uint32_t)R[1], (uint32_t)R[0], 0x05010400u), t23 = perm((uint32_t)R[3], (uint32_t)R[2], 0x05010400u);
    return perm(t23, t01, 0x05040100u);
}

// diagnostics (MIMC3_MX_STATS): phase clocks stay in scalar registers and are stored once, by MIMC3_MX_STATS_OUT, before the kernel's normal exit
#define MIMC3_MX_STAMP(i)                                                                      \
    if (p.stats) {                                                                             \
        const unsigned long long t_now = __builtin_amdgcn_s_memtime();                         \
        t_ph[i] = t_now - t_prev;                                                              \
        t_prev = t_now;                                                                        \
    }
#define MIMC3_MX_STATS_OUT                                                                     \
    if (p.stats && lane == 0) { _Pragma("unroll") for (int i_ = 0; i_ < 7; i_++) p.stats[kStatW * (size_t)blockIdx.x + i_] = t_ph[i_]; }


template <class C>
__global__ __launch_bounds__(C::NT, C::MINW) void match_ncc_dlc_mx(MatchU8Args p)
{
    constexpr int OCW = C::OCW, CW = C::CW, NPX = C::NPX, KCW = C::KCW, KCV = C::KCV, NTR = C::NTR, PW = C::PW, CP = C::CP, CH0 = C::CH0, VP = C::VP, NT = C::NT;
    constexpr bool GEN = C::GEN;
    __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS];
    unsigned char *WT = smem;
    float *val = reinterpret_cast<float *>(smem);                       // [32][VP] NCC surface (over the tile, once it is consumed)
    unsigned char *CH = smem + C::OFF_CH;                               // chip planes
    uint32_t *vis = reinterpret_cast<uint32_t *>(smem + C::OFF_VIS);    // visited bits of the 32 tile rows
    unsigned long long t_prev = p.stats ? __builtin_amdgcn_s_memtime() : 0ull;
    unsigned long long t_ph[7] = {0, 0, 0, 0, 0, 0, 0};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int gidx = blockIdx.x;
    [[maybe_unused]] int rpos = 0;                           // REC: the list position, i.e. where the point's record is
    [[maybe_unused]] uint32_t recw = 0u;                     // REC: lane k < 16 holds dword k of the record
    auto rec = [&](int k) __attribute__((always_inline)) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)recw, k); };
    auto rec64 = [&](int k) __attribute__((always_inline)) -> unsigned long long { return ((unsigned long long)rec(k + 1) << 32) | rec(k); };
    // REC: the launch goes on into the advance list of u8_classify -- rest points whose window holds nulls, but none in the climb area
    // (mx_climb_area, match_kernel.h).  Workgroup cnt + i takes the point at rest position advance[i], from its rest record; it finishes
    // the point only if every scan stays inside the area, and then marks the record done for the register-tiled launch (kRecDone)
    [[maybe_unused]] bool adv = false;
    if (C::REC || p.point_list) {                            // list mode: the clean list of u8_classify (the launch is sized for all N points)
        int cnt = *p.point_count;
        if constexpr (C::REC) {
            if (gidx >= cnt) {                               // (clean and advance points are disjoint: the N-sized grid holds both)
                gidx -= cnt; cnt = p.point_count[2]; adv = true;
            }
        }
        if (gidx >= cnt) return;
        const int per = cnt >> 3;
        if (gidx < per * 8) gidx = (gidx & 7) * per + (gidx >> 3);              // XCD-contiguous order of the list positions
        if constexpr (C::REC) {
            static_assert(sizeof(U8PointRec) == 64 && offsetof(U8PointRec, rowQ) == 56, "the dword numbers below");
            rpos = adv ? (p.rest_list + p.N)[gidx] : gidx;
            recw = reinterpret_cast<const uint32_t *>((adv ? p.rest_recs : p.point_recs) + rpos)[lane & 15];
            gidx = (int)rec(0);
            if (adv && p.stats && tid == 0) p.stats[kStatW * (size_t)blockIdx.x + 7] = 1ull;      // diagnostics: tried
        } else gidx = p.point_list[gidx];
    } else {
        const int nb = gridDim.x, per = nb >> 3;
        if (per > 0 && gidx < per * 8) gidx = (gidx & 7) * per + (gidx >> 3);   // XCD-contiguous point order
    }
    if (!C::REC && gidx >= p.N) return;
    if (!C::REC && p.point_flags && p.point_flags[gidx] != (uint8_t)p.flag_value) return;      // flag mode: the points another kernel handed over
    auto hand_on = [&](uint8_t to) __attribute__((always_inline)) {
        if constexpr (C::REC) {
            if (adv) return;                                 // an advance point that cannot finish is on the rest list already, class and record
            // the point goes to the rest list with its record, which holds all the register-tiled kernel's header reads: fetched again
            // (a few dozen points per launch) rather than carried through the kernel in a register.  Wave 0 calls this, whole
            if (wave == 0) {
                int slot = 0;
                if (lane == 0) {
                    p.mx_flags[gidx] = to;
                    if (to == kMxRest) { slot = atomicAdd(p.rest_count, 1); p.rest_list[slot] = gidx; }
                }
                slot = __builtin_amdgcn_readfirstlane(slot);
                if (to == kMxRest && lane < 16)
                    reinterpret_cast<uint32_t *>(p.rest_recs + slot)[lane] = reinterpret_cast<const uint32_t *>(p.point_recs + rpos)[lane];
            }
        } else if (tid == 0) {
            p.mx_flags[gidx] = to;
            if (!C::FULL && p.mx_classified && to == kMxRest) p.rest_list[atomicAdd(p.rest_count, 1)] = gidx;
        }
    };

    const unsigned char *chip_pl = p.swap ? p.p1 : p.p0;
    const unsigned char *win_pl = p.swap ? p.p0 : p.p1;
    const int Wp = p.Wp, PAD = p.pad;
    // SURF: a point that leaves before its surface exists gets an all-NaN one, as the float kernel's (both waves store)
    auto surf_nan = [&]() __attribute__((always_inline)) {
        if constexpr (C::SURF) {
            const int NC = (2 * p.full_R + 1) * (2 * p.full_R + 1);
            float *sf = p.full_surf + (size_t)gidx * (size_t)NC;
            for (int k = tid; k < NC; k += NT) sf[k] = __builtin_nanf("");
        }
    };

    // ---- point header (as match_px_kernel.hip) ---------------------------------------------------------------------
    // (REC: u8_classify has read and derived all of it; the record's dwords by number, see U8PointRec)
    int u0, v0;
    if constexpr (C::REC) { u0 = (int)rec(1); v0 = (int)rec(2); }
    else {
        const double *row = p.xyuvav + (size_t)p.xy_stride * (size_t)gidx + p.xy_col;
        u0 = (int)row[0]; v0 = (int)row[1];
    }
    // (full mode, a point that breaks the bounds mimc3_match_ncc_full refuses -- only the _dev entry can pass one: no read, all NaN)
    if (C::FULL && (u0 - OCW < 0 || u0 + OCW >= p.W || v0 - OCW < 0 || v0 + OCW >= p.H)) {
        if (tid == 0) { full_store(p.out + 8 * (size_t)gidx, __builtin_nanf("")); full_peak_store<C>(p, gidx, -1); full_cand_fill<C>(p, gidx, __builtin_nanf("")); }
        surf_nan();
        return;
    }
    int64_t pbeg;
    int npiv;
    if constexpr (C::REC) { pbeg = (int64_t)rec64(6); npiv = (int)(rec(5) & kRecNpivMask); }
    else {
        pbeg = C::FULL ? 0 : p.piv_off[gidx];
        npiv = C::FULL ? 1 : (int)(p.piv_off[gidx + 1] - pbeg);
    }
    const int32_t *pv_g = p.piv_uv + 2 * pbeg;
    // Everything the header needs from memory beyond (u, v) and the pivot range is issued together -- the last pivot, the twelve table
    // corners of the three chip-side queries (one per lane), the chip's corner pixel, this lane's pivot -- and only then waited for:
    // one memory round trip instead of one per query (the values are wave-uniform, but the kernel stores to global memory, so the
    // compiler loads them through the vector path and every readfirstlane is a wait).
    const int cu0 = u0 - OCW + PAD, cv0 = v0 - OCW + PAD;                       // plane position of chip pixel (0, 0)
    typedef unsigned long long SatT;
    const SatT *sat_chip = reinterpret_cast<const SatT *>(p.swap ? p.sat1 : p.sat0);
    const SatT *sat_win = reinterpret_cast<const SatT *>(p.swap ? p.sat0 : p.sat1);
    // (full mode: the point's shift in place of the last pivot)
    int2 lastpv = make_int2(0, 0);
    if constexpr (!C::REC)
        lastpv = C::FULL ? (p.full_shift ? *reinterpret_cast<const int2 *>(p.full_shift + 2 * (size_t)gidx) : make_int2(0, 0))
                         : *reinterpret_cast<const int2 *>(pv_g + 2 * (npiv - 1));
    SatT satv = 0;
    if constexpr (!C::REC) {   // lane 4 q + c: corner c of query q (0: the chip, 1: its last column, 2: its last row)
        const int q = (lane >> 2) & 3, c = lane & 3;
        const int bx = cu0 + (q == 1 ? CW - 1 : 0), by = cv0 + (q == 2 ? CW - 1 : 0), bw = q == 1 ? 1 : CW, bh = q == 2 ? 1 : CW;
        if (lane < 12) satv = sat_chip[(size_t)(by + ((c & 2) ? bh : 0)) * p.sat_ws + bx + ((c & 1) ? bw : 0)];
    }
    uint32_t cornerv = 0u;
    if constexpr (!C::REC) cornerv = chip_pl[(size_t)(cv0 + CW - 1) * Wp + cu0 + CW - 1];
    // the pivots (lane k of wave 0 = pivot k in the climbs): parked in LDS until the surface is there
    int2 pv_mine = make_int2(0, 0);
    if (!C::FULL && wave == 0 && lane < npiv && npiv <= 64) pv_mine = *reinterpret_cast<const int2 *>(pv_g + 2 * lane);
    // ... and the first batch of the chip's pixels (aligned dwords of its rows; written to LDS once the tile is on its way)
    constexpr int CD = C::CD, CTASK = CW * CD, CNIT = (CTASK + NT - 1) / NT, CKB = CNIT < 5 ? CNIT : 5;
    const int csh = cu0 & 3;
    const uint32_t *cgb = reinterpret_cast<const uint32_t *>(chip_pl + (size_t)cv0 * Wp + (cu0 - csh));
    uint32_t clo[CKB], chi[CKB];
    auto chip_loads = [&](int it0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < CKB; k++) {
            const int t = tid + NT * (it0 + k);
            const int r = t / CD, j = t - CD * r;
            const bool on = (it0 + k < CNIT) && t < CTASK;
            const uint32_t go = (uint32_t)(on ? r : 0) * (uint32_t)(Wp >> 2) + (uint32_t)(on ? j : 0);      // (32-bit offsets from a uniform base)
            clo[k] = cgb[go]; chi[k] = cgb[go + 1u];
        }
    };
    chip_loads(0);
    const int lu = C::REC ? (int)rec(3) : __builtin_amdgcn_readfirstlane(lastpv.x), lv = C::REC ? (int)rec(4) : __builtin_amdgcn_readfirstlane(lastpv.y);
    // (full mode: the search box is the Dx2 x Dy2 window centred on c, i.e. dx2 = dy2 = R + OCW; the tile's cell s_t = s + R)
    const int dx2 = C::FULL ? p.full_R + OCW : (lu < 0 ? -lu : lu) + OCW + 2, dy2 = C::FULL ? p.full_R + OCW : (lv < 0 ? -lv : lv) + OCW + 2;
    const int Dx2 = 2 * dx2 + 1, Dy2 = 2 * dy2 + 1;
    const int csx = Dx2 - 2 * OCW + 1, csy = Dy2 - 2 * OCW + 1;          // compact cells; a climb touches [1, cs - 2]
    const int wu0 = u0 + p.off_u - dx2 + PAD + (C::FULL ? lu : 0), wv0 = v0 + p.off_v - dy2 + PAD + (C::FULL ? lv : 0);   // plane position of window pixel (0, 0)
    if (C::FULL && (wu0 < 0 || wv0 < 0 || wu0 + Dx2 > p.W + 2 * PAD || wv0 + Dy2 > p.H + 2 * PAD)) {
        if (tid == 0) { full_store(p.out + 8 * (size_t)gidx, __builtin_nanf("")); full_peak_store<C>(p, gidx, -1); full_cand_fill<C>(p, gidx, __builtin_nanf("")); }
        surf_nan();
        return;
    }
    // ---- what this kernel takes -----------------------------------------------------------------------------------
    // the tile: all reachable cells if they fit, else centred on the pivots' starts (a scan that leaves it hands the point on)
    int tx0, ty0;
    bool fits;
    [[maybe_unused]] uint32_t area_w = 0u, tile_w = 0u;      // REC: the record's dwords with the climb area / the done bit, kept in scalar registers
    if constexpr (C::REC) {
        const uint32_t t = rec(8);
        tx0 = (int)(t & 1023u); ty0 = (int)((t >> 10) & 1023u); fits = ((t >> 20) & 1u) != 0u;
        area_w = rec(5); tile_w = t;
    }
    else fits = mx_tile_fit(lu, lv, OCW, dx2, dy2, csx, csy, C::FULL ? 0 : 1, tx0, ty0);
    // the null count of the window's written area (:869-886) and the first batch of the tile's pixels: issued now, read below
    int win_nulls_v = 0;
    if constexpr (!C::REC) win_nulls_v = sat_nulls_u8(sat_win, p.sat_ws, wu0, wv0, C::FULL ? Dx2 : 2 * dx2, C::FULL ? Dy2 : 2 * dy2, lane);      // (exact for any window size; full mode: the whole search box)
    constexpr int NSEG = C::SW / 16, TTASK = C::KW * NSEG;           // (tile rows >= KW and columns >= SW are only ever weighted 0: left as they are)
    constexpr int TNIT = (TTASK + NT - 1) / NT, TKB = TNIT < 4 ? TNIT : 4;
    const int tsh = (wu0 + tx0) & 3;
    const uint32_t *tgb = reinterpret_cast<const uint32_t *>(win_pl + (size_t)(wv0 + ty0) * Wp + (wu0 + tx0 - tsh));
    uint32_t td[TKB][5];
    // (full mode: the tile reaches up to 31 - 2R rows and 50 - 2R columns past the search box, which may end at the plane's last row:
    //  the loads are clamped to the plane; what a clamped load brings only reaches cells outside the search range)
    const uint32_t tlim = C::FULL ? (uint32_t)(((size_t)(p.H + 2 * PAD) * (size_t)Wp - ((size_t)(wv0 + ty0) * Wp + (size_t)(wu0 + tx0 - tsh))) / 4 - 1) : 0u;
    (void)tlim;
    auto tile_loads = [&](int it0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < TKB; k++) {
            const int t = tid + NT * (it0 + k);
            const int y = t / NSEG, q = t - NSEG * y;
            const bool on = (it0 + k < TNIT) && t < TTASK;
            const uint32_t go = (uint32_t)(on ? y : 0) * (uint32_t)(Wp >> 2) + 4u * (uint32_t)(on ? q : 0);
#pragma unroll
            for (int j = 0; j < 5; j++) td[k][j] = tgb[C::FULL ? min(go + (uint32_t)j, tlim) : go + (uint32_t)j];
        }
    };
    tile_loads(0);
    // the chip's sums and null count, and -- for the closed-form T4 terms -- those of its last column and last row
    auto lane64 = [&](int l) __attribute__((always_inline)) -> SatT {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)satv, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(satv >> 32), l);
        return ((SatT)hi << 32) | lo;
    };
    const SatT chipQ = C::REC ? rec64(10) : lane64(3) - lane64(1) - lane64(2) + lane64(0);
    const SatT colQ = C::REC ? rec64(12) : lane64(7) - lane64(5) - lane64(6) + lane64(4);
    const SatT rowQ = C::REC ? rec64(14) : lane64(11) - lane64(9) - lane64(10) + lane64(8);
    const uint32_t corner = C::REC ? rec(8) >> 24 : (uint32_t)__builtin_amdgcn_readfirstlane((int)cornerv);

    const int chip_nulls = (int)(chipQ >> kSatNullShift8);
    const int win_nulls = C::REC ? (int)rec(9) : __builtin_amdgcn_readfirstlane(win_nulls_v);
    // (behind u8_classify these two tests never fire on a listed point -- they are its own, from the same helpers; they stay as the
    //  guard of a launch whose list did not come from it.  The guard decides who computes the point, it does not protect the loads
    //  above: the last pivot was read at pv_g + 2 (npiv - 1) before it, so a point without pivots has already read 8 bytes in front
    //  of its range, as it always did -- the C ABI refuses empty pivot lists, and the classifier tests npiv before it reads)
    if (!mx_takes(npiv, fits)) { hand_on(kMxRest); return; }
    if (!GEN) {
        // (an advance point: its window's nulls lie outside its climb area, the chip's guard stays)
        const uint8_t cls = mx_null_class((C::REC && adv) ? 0 : win_nulls, chip_nulls, p.mx_wn_on, p.mx_gen_on);
        if (cls != 0) { hand_on(cls); return; }
    }
    // general form: wn = the written area of the window holds nulls (then the never-written last row / column are nulls like any other,
    // else they are applied in closed form as in the clean form); cn = the chip holds nulls
    const bool wn = GEN && win_nulls != 0, cn = C::CN && chip_nulls != 0;

    // ---- validity (a6, :605-644): nulls of the chip / of the whole Dy2 x Dx2 search area (its last row and column are never written: zeros)
    if constexpr (C::FULL) {                                  // (the search box has no never-written row or column)
        const float max_ratio = 0.8f;
        const float rc = (float)chip_nulls / (float)NPX;
        const float rw = (float)win_nulls / (float)(Dx2 * Dy2);
        if (rc > max_ratio || rw > max_ratio) {
            if (tid == 0) { full_store(p.out + 8 * (size_t)gidx, -3.0f); full_peak_store<C>(p, gidx, -1); full_cand_fill<C>(p, gidx, -3.0f); }
            surf_nan();
            return;
        }
    } else {
        const float max_ratio = 0.8f;
        const float rc = (float)chip_nulls / (float)NPX;
        const float rw = (float)(win_nulls + Dx2 + Dy2 - 1) / (float)(Dx2 * Dy2);
        if (rc > max_ratio || rw > max_ratio) {
            if (C::REC && adv) return;                        // (left to the register-tiled launch, which counts the nulls it stages)
            if (tid == 0) {
                const float nanv = __builtin_nanf("");
                p.out[3 * (size_t)gidx + 0] = nanv; p.out[3 * (size_t)gidx + 1] = nanv; p.out[3 * (size_t)gidx + 2] = -3.0f;
            }
            return;
        }
    }
    const uint32_t SX = (uint32_t)chipQ & ((1u << kSatSqShift8) - 1u);
    const uint32_t SXX = (uint32_t)(chipQ >> kSatSqShift8) & ((1u << (kSatNullShift8 - kSatSqShift8)) - 1u);

    // ---- stage the tile: window pixels (tx0 + x, ty0 + y), x < SW, y < KW, as signed bytes b - 128 (both waves) ---------------
    {
#pragma unroll 1
        for (int it0 = 0; it0 < TNIT; it0 += TKB) {
            if (it0 > 0) tile_loads(it0);
#pragma unroll
            for (int k = 0; k < TKB; k++) {
                const int t = tid + NT * (it0 + k);
                const int y = t / NSEG, q = t - NSEG * y;
                if ((it0 + k < TNIT) && t < TTASK) {
                    uint4 w;
                    w.x = alignb(td[k][1], td[k][0], tsh) ^ 0x80808080u;
                    w.y = alignb(td[k][2], td[k][1], tsh) ^ 0x80808080u;
                    w.z = alignb(td[k][3], td[k][2], tsh) ^ 0x80808080u;
                    w.w = alignb(td[k][4], td[k][3], tsh) ^ 0x80808080u;
                    *reinterpret_cast<uint4 *>(WT + y * PW + 16 * q) = w;
                    if (C::ZPL && wn) *reinterpret_cast<uint4 *>(smem + C::OFF_Z + y * PW + 16 * q) = make_uint4(null80(w.x), null80(w.y), null80(w.z), null80(w.w));
                }
            }
        }
    }
    // ---- chip planes: zeros, then CW rows of (a ^ 0x80) [and of the two byte planes of a^2] -------------------------------
    {
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < (C::NPL * C::CHB) / 16; i += NT) reinterpret_cast<uint4 *>(CH)[i] = z4;
        if (wave == 0) reinterpret_cast<int2 *>(smem + C::OFF_PIV)[lane] = pv_mine;
        if (GEN && tid < 4) reinterpret_cast<uint32_t *>(smem + C::OFF_RM)[tid] = 0u;
    }
    __syncthreads();
    {
        // T4: the search area's last column and last row are never written (:869-886): nulls.  (What lies beyond them inside the tile
        // only reaches cells no climb can touch.)
        const int zx = C::FULL ? C::SW : Dx2 - 1 - tx0, zy = C::FULL ? C::KW : Dy2 - 1 - ty0;    // (full mode: none)
        if (zx < C::SW) for (int y = tid; y < C::KW; y += NT) { WT[y * PW + zx] = 0x80; if (C::ZPL && wn) smem[C::OFF_Z + y * PW + zx] = 0x80; }
        if (zy < C::KW) for (int x = tid; x < C::SW / 4; x += NT) {
            *reinterpret_cast<uint32_t *>(WT + zy * PW + 4 * x) = 0x80808080u;
            if (C::ZPL && wn) *reinterpret_cast<uint32_t *>(smem + C::OFF_Z + zy * PW + 4 * x) = 0x80808080u;
        }
        constexpr uint32_t LASTM = C::LASTN >= 4 ? 0xffffffffu : ((1u << (8 * C::LASTN)) - 1u);
#pragma unroll 1
        for (int it0 = 0; it0 < CNIT; it0 += CKB) {
            if (it0 > 0) chip_loads(it0);
#pragma unroll
            for (int k = 0; k < CKB; k++) {
                const int t = tid + NT * (it0 + k);
                const int r = t / CD, j = t - CD * r;
                if ((it0 + k < CNIT) && t < CTASK) {
                    const uint32_t a = alignb(chi[k], clo[k], csh);
                    const uint32_t m = (j == CD - 1) ? LASTM : 0xffffffffu;
                    *reinterpret_cast<uint32_t *>(CH + CH0 + CP * r + 4 * j) = (a ^ 0x80808080u) & m;
                    if (GEN && wn) {                          // the byte planes of a^2
                        uint32_t l, g;
                        squares_dword(a, l, g);
                        *reinterpret_cast<uint32_t *>(CH + C::CHB + CH0 + CP * r + 4 * j) = (l ^ 0x80808080u) & m;
                        *reinterpret_cast<uint32_t *>(CH + 2 * C::CHB + CH0 + CP * r + 4 * j) = (g ^ 0x80808080u) & m;
                    }
                    if (GEN && cn) {                          // a null pixel (DN 0) among the dword's chip pixels: flag the chip row
                        const uint32_t nz = (((a & 0x7f7f7f7fu) + 0x7f7f7f7fu) | a) & 0x80808080u & m;
                        if (nz != (0x80808080u & m)) atomicOr(reinterpret_cast<uint32_t *>(smem + C::OFF_RM) + (r >> 5), 1u << (r & 31));
                    }
                }
            }
        }
    }
    __syncthreads();
    MIMC3_MX_STAMP(0)

    // lane (n, h) of wave w: cell column s = 16 w + n; byte i of K chunk c <-> window column 16 w + 64 c + 16 h + i
    const int n = lane & 15, h = lane >> 4;
    const unsigned char *arow = WT + band_row(n) * PW + 16 * wave + 16 * h;      // A operand: tile row r + 16 mt + band_row(n)
    const int boff = CH0 + 16 * h - n;                                   // B operand: chip-row bytes 64 c + 16 h - n + i
    const uint32_t bsh = (uint32_t)boff & 3u;
    const unsigned char *brow = CH + (boff & ~3);

    // ---- the product surface (and the null corrections) ------------------------------------------------------------------
    //      Software-pipelined by hand: the LDS reads of chip row r + 1 are in flight while row r's MFMAs issue (left to the compiler,
    //      every row waited for its own reads: one LDS latency per row).  No branch inside the loop: with conditional reads the
    //      compiler's wait counts assume the shorter queue; an odd chip is followed by an all-zero row, whose products add nothing.
    const v4i zero4 = {0, 0, 0, 0};
    // accumulators (two 16 x 16 tiles each): sum a'b'; general form, window nulls zb = [b == 0]: sum zb a', sum zb (a^2 & 255)', sum zb (a^2 >> 8)';
    // chip nulls za = [a == 0]: sum b' za, sum (b^2 & 255)' za, sum (b^2 >> 8)' za, and sum zb za
    v4i acc[2] = {zero4, zero4}, accz[2] = {zero4, zero4}, accl[2] = {zero4, zero4}, acch[2] = {zero4, zero4};
    v4i accy[2] = {zero4, zero4}, accyl[2] = {zero4, zero4}, accyh[2] = {zero4, zero4}, acczz[2] = {zero4, zero4};
    (void)accz; (void)accl; (void)acch; (void)accy; (void)accyl; (void)accyh; (void)acczz;
    {
        // general form: which chip rows hold nulls (their Toeplitz rows are the only ones the chip-null correlations need)
        uint32_t rm0 = 0, rm1 = 0, rm2 = 0;
        if (GEN && cn) {
            const uint32_t *rmp = reinterpret_cast<const uint32_t *>(smem + C::OFF_RM);
            rm0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rmp[0]); rm1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rmp[1]);
            rm2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rmp[2]);
        }
        auto row_has_null = [&](int r) __attribute__((always_inline)) -> bool {
            const uint32_t w = r < 32 ? rm0 : (r < 64 ? rm1 : rm2);
            return ((w >> (r & 31)) & 1u) != 0u;
        };
        const unsigned char *zrow = smem + C::OFF_Z + (arow - WT);         // the null plane under the lane's A operand (ZPL)
        (void)zrow;
        // (double-buffered across rows: the tile rows and the a' plane.  The general form's other operands -- the a^2 planes, the null plane --
        //  are read at the start of a row's turn and used at its end, behind the MFMAs that do not need them: half the operand registers)
        struct RowOps { v4i a[2][KCW]; uint32_t d[KCW][5]; };
        auto issue = [&](int r, RowOps &o) __attribute__((always_inline)) {
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int c = 0; c < KCW; c++) o.a[m][c] = *reinterpret_cast<const v4i *>(arow + (r + 16 * m) * PW + 64 * c);
#pragma unroll
            for (int c = 0; c < KCW; c++) {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(brow + CP * r + 64 * c);
#pragma unroll
                for (int k = 0; k < 5; k++) o.d[c][k] = q[k];
            }
        };
        auto shifted = [&](const uint32_t (&d)[KCW][5], v4i (&b)[KCW]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < KCW; c++)
#pragma unroll
                for (int k = 0; k < 4; k++) b[c][k] = (int)alignb(d[c][k + 1], d[c][k], bsh);
        };
        // (the null-plane operands are 0x80 = -128 per null: their correlations come out times -128, their product times 16384)
        auto consume = [&](const RowOps &o, int r) __attribute__((always_inline)) {
            [[maybe_unused]] uint32_t d1[KCW][5], d2[KCW][5];
            [[maybe_unused]] v4i az[2][KCW];
            if constexpr (GEN) {
#pragma unroll
                for (int c = 0; c < KCW; c++) {
                    const uint32_t *q1 = reinterpret_cast<const uint32_t *>(brow + C::CHB + CP * r + 64 * c), *q2 = reinterpret_cast<const uint32_t *>(brow + 2 * C::CHB + CP * r + 64 * c);
#pragma unroll
                    for (int k = 0; k < 5; k++) { d1[c][k] = q1[k]; d2[c][k] = q2[k]; }
                }
                if constexpr (C::ZPL) {
#pragma unroll
                    for (int m = 0; m < 2; m++)
#pragma unroll
                        for (int c = 0; c < KCW; c++) az[m][c] = *reinterpret_cast<const v4i *>(zrow + (r + 16 * m) * PW + 64 * c);
                }
            }
            v4i b[KCW];
            shifted(o.d, b);
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int c = 0; c < KCW; c++) acc[m] = mfma(o.a[m][c], b[c], acc[m]);
            if constexpr (GEN) {
                const bool cnrow = cn && row_has_null(r);
                v4i z[2][KCW];
                if (wn) {
#pragma unroll
                    for (int m = 0; m < 2; m++)
#pragma unroll
                        for (int c = 0; c < KCW; c++) {
                            if constexpr (C::ZPL) z[m][c] = az[m][c]; else z[m][c] = null80v(o.a[m][c]);
                            accz[m] = mfma(z[m][c], b[c], accz[m]);
                        }
                }
                if (cnrow) {
#pragma unroll
                    for (int c = 0; c < KCW; c++) {
                        const v4i za = null80v(b[c]);              // (a padding byte is 0x00, a null chip pixel 0x80)
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            v4i lo, hi;
                            squares(o.a[m][c], lo, hi);
                            accy[m] = mfma(o.a[m][c], za, accy[m]); accyl[m] = mfma(lo, za, accyl[m]); accyh[m] = mfma(hi, za, accyh[m]);
                            if (wn) acczz[m] = mfma(z[m][c], za, acczz[m]);
                        }
                    }
                }
                if (wn) {
                    v4i bq[KCW];
                    shifted(d1, bq);
#pragma unroll
                    for (int m = 0; m < 2; m++)
#pragma unroll
                        for (int c = 0; c < KCW; c++) accl[m] = mfma(z[m][c], bq[c], accl[m]);
                    shifted(d2, bq);
#pragma unroll
                    for (int m = 0; m < 2; m++)
#pragma unroll
                        for (int c = 0; c < KCW; c++) acch[m] = mfma(z[m][c], bq[c], acch[m]);
                }
            }
        };
        RowOps o0, o1;
        issue(0, o0);
#pragma unroll 1
        for (int r = 0; r < C::CWE; r += 2) {
            issue(r + 1, o1);
            __builtin_amdgcn_sched_barrier(0);
            consume(o0, r);
            __builtin_amdgcn_sched_barrier(0);
            issue(r + 2 < C::CWE ? r + 2 : r + 1, o0);          // (the last trip re-reads a row: nothing consumes it)
            __builtin_amdgcn_sched_barrier(0);
            consume(o1, r + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (GEN) {        // the two byte planes of each squared operand back into one sum (and out of the -128 scale): 16 registers fewer from here on
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                accl[m][i] = ((-accl[m][i]) >> 7) + 256 * ((-acch[m][i]) >> 7);
                accyl[m][i] = ((-accyl[m][i]) >> 7) + 256 * ((-accyh[m][i]) >> 7);
            }
    }
    MIMC3_MX_STAMP(1)

    // ---- window-side box sums of the wave's 32 x 16 cells: sum b, sum b^2 (and the null count) ------------------------------------
    //      row-box sums R[y][s] = sum_{x = s}^{s + CW - 1} q[y][x] by MFMA (A = 16 tile rows, B = the band of ones), then
    //      Box[dy][s] = sum_{y = dy}^{dy + CW - 1} R[y][s] by MFMA (A = the band of ones, B = the byte planes of R: the four registers
    //      of a 16-row accumulator tile are one dword of the B operand -- the accumulator layout has R's rows where B has its K index)
    v4i boxb[2], boxq[2], boxz[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    [[maybe_unused]] uint32_t bands_t = 0xffu;               // BOXT: the bands the finish will run (wave-uniform)
    if constexpr (C::BOXT) {
        // From the window plane's packed table (built once per image): the sums depend on the plane and the box position alone.  Only
        // the cells of the bands the finish will run -- a wave whose columns miss the climb area loads nothing -- four entries per cell
        // at 32-bit offsets from the entry of the tile's pixel (0, 0), the four bands of an accumulator tile in flight together, each
        // cell combined to its two sums as its entries arrive.  The never-written last column and row (T4) are zeros of the staged tile
        // but real pixels of the table: sat_cell_corners ends such a box in front of them.  Exact integers, the same as the MFMAs'
        const uint32_t ar = area_w >> 8, w = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
        const uint32_t x0 = ar & 31u, x1 = (ar >> 5) & 31u, y0 = (ar >> 10) & 31u, y1 = (ar >> 15) & 31u;
        bands_t = (w >= (x0 >> 4) && w <= (x1 >> 4)) ? ((2u << (y1 >> 2)) - (1u << (y0 >> 2))) & 0xffu : 0u;
        const int zx = Dx2 - 1 - tx0, zy = Dy2 - 1 - ty0, xl = csx - 2 - tx0, yl = csy - 2 - ty0;
        const uint32_t ws8 = 8u * (uint32_t)p.sat_ws;
        const unsigned char *sb = reinterpret_cast<const unsigned char *>(sat_win + (size_t)(wv0 + ty0) * p.sat_ws + (wu0 + tx0));
#pragma unroll
        for (int m = 0; m < 2; m++) {
            SatT q[4][4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (!((bands_t >> (4 * m + i)) & 1u)) continue;
                uint32_t o[4];
                sat_cell_corners(16 * wave + n, 16 * m + 4 * i + h, CW, xl, yl, zx, zy, ws8, o);
#pragma unroll
                for (int c = 0; c < 4; c++) q[i][c] = *reinterpret_cast<const SatT *>(sb + o[c]);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (!((bands_t >> (4 * m + i)) & 1u)) continue;
                int s, ss;
                sat_u8_sums(q[i][3] - q[i][1] - q[i][2] + q[i][0], s, ss);
                asm volatile("" : "+v"(s), "+v"(ss));         // (formed here: the finish carries two registers per cell, not eight)
                boxb[m][i] = s; boxq[m][i] = ss;
            }
        }
    } else {
        const Bands<CW, KCW, KCV> &bd = kBands<CW, KCW, KCV>;
        v4i hb[KCW];
#pragma unroll
        for (int c = 0; c < KCW; c++) hb[c] = *reinterpret_cast<const v4i *>(&bd.hb[c][lane][0]);
        auto tile_a = [&](int t, v4i (&a)[KCW]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < KCW; c++) a[c] = *reinterpret_cast<const v4i *>(arow + 16 * t * PW + 64 * c);
        };
        {   // sum b (and the null count)
            v4i p0[KCV], p1[KCV], pz[KCV];
#pragma unroll
            for (int t = 0; t < 4 * KCV; t++) {
                uint32_t q0 = 0, q1 = 0, qz = 0;
                if (t < NTR) {
                    v4i a[KCW];
                    tile_a(t, a);
                    v4i R = zero4;
#pragma unroll
                    for (int c = 0; c < KCW; c++) R = mfma(a[c], hb[c], R);
#pragma unroll
                    for (int i = 0; i < 4; i++) R[i] += 128 * CW;
                    planes2(R, q0, q1);
                    if (GEN && wn) {                          // the row counts of the nulls (the null plane is -128 per null)
                        v4i Z = zero4;
#pragma unroll
                        for (int c = 0; c < KCW; c++) {
                            v4i zc;
                            if constexpr (C::ZPL) zc = *reinterpret_cast<const v4i *>(smem + C::OFF_Z + (arow - WT) + 16 * t * PW + 64 * c);
                            else zc = null80v(a[c]);
                            Z = mfma(zc, hb[c], Z);
                        }
#pragma unroll
                        for (int i = 0; i < 4; i++) Z[i] = (-Z[i]) >> 7;
                        qz = planes1(Z);
                    }
                }
                p0[t >> 2][t & 3] = (int)q0; p1[t >> 2][t & 3] = (int)q1; pz[t >> 2][t & 3] = (int)qz;
            }
#pragma unroll
            for (int m = 0; m < 2; m++) {
                v4i v0 = zero4, v1 = zero4;
#pragma unroll
                for (int c = 0; c < KCV; c++) {
                    const v4i vb = *reinterpret_cast<const v4i *>(&bd.vb[m][c][lane][0]);
                    v0 = mfma(vb, p0[c], v0); v1 = mfma(vb, p1[c], v1);
                    if (GEN && wn) boxz[m] = mfma(vb, pz[c], boxz[m]);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) boxb[m][i] = (v0[i] + 128 * CW) + 256 * (v1[i] + 128 * CW);
            }
        }
        {   // sum b^2
            v4i p0[KCV], p1[KCV], p2[KCV];
#pragma unroll
            for (int t = 0; t < 4 * KCV; t++) {
                uint32_t q0 = 0, q1 = 0, q2 = 0;
                if (t < NTR) {
                    v4i a[KCW];
                    tile_a(t, a);
                    v4i Rl = zero4, Rh = zero4;
#pragma unroll
                    for (int c = 0; c < KCW; c++) {
                        v4i lo, hi;
                        squares(a[c], lo, hi);
                        Rl = mfma(lo, hb[c], Rl); Rh = mfma(hi, hb[c], Rh);
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) Rl[i] = (Rl[i] + 128 * CW) + 256 * (Rh[i] + 128 * CW);
                    planes3(Rl, q0, q1, q2);
                }
                p0[t >> 2][t & 3] = (int)q0; p1[t >> 2][t & 3] = (int)q1; p2[t >> 2][t & 3] = (int)q2;
            }
#pragma unroll
            for (int m = 0; m < 2; m++) {
                v4i v0 = zero4, v1 = zero4, v2 = zero4;
#pragma unroll
                for (int c = 0; c < KCV; c++) {
                    const v4i vb = *reinterpret_cast<const v4i *>(&bd.vb[m][c][lane][0]);
                    v0 = mfma(vb, p0[c], v0); v1 = mfma(vb, p1[c], v1); v2 = mfma(vb, p2[c], v2);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) boxq[m][i] = (v0[i] + 128 * CW) + 256 * (v1[i] + 128 * CW) + 65536 * (v2[i] + 128 * CW);
            }
        }
    }

    if constexpr (C::REC && !C::BOXT) {      // (formed here: left alone, the compiler sinks these sums into the finish's skippable bands and carries their byte planes there)
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) asm volatile("" : "+v"(boxb[m][i]), "+v"(boxq[m][i]));
    }
    MIMC3_MX_STAMP(2)
    __syncthreads();                                        // the tile's bytes become the NCC surface

    // ---- NCC of the 8 cells of this lane (:734): exact integer sums, the f64 formula rounded to f32 ------------------------------
    //   reference:  (float)( num / sqrt(P) ),  num = n sxy - sx sy  and  va = n sxx - sx^2,  vb = n syy - sy^2  exact integers in f64,
    //               P = va * vb rounded once, sqrt and the division correctly rounded: the f64 quotient Qd is within 2^-51 of num / sqrt(P).
    //   here:       ncc_quot_fast (match_full_tail.h: the refined reciprocal square root), and for the 2^-15 of the cells it reports as too
    //               close to an f32 rounding boundary, or whose P is not positive, ncc_quot_exact: the reference's own operations.
    {
        uint32_t tix = threadIdx.x;
        asm volatile("" : "+v"(tix));                        // (formed again from the thread index: carried over from the header, it was the one register that spilled)
        const int sx_col = (int)(tix >> 6) * 16 + (int)(tix & 15u), cx = tx0 + sx_col;
        // clean form, T4 in closed form: a cell whose box reaches the never-written last column (row) loses the chip's last column (row)
        uint32_t cS = (uint32_t)colQ & ((1u << kSatSqShift8) - 1u), cSS = (uint32_t)(colQ >> kSatSqShift8) & ((1u << (kSatNullShift8 - kSatSqShift8)) - 1u);
        uint32_t rS = (uint32_t)rowQ & ((1u << kSatSqShift8) - 1u), rSS = (uint32_t)(rowQ >> kSatSqShift8) & ((1u << (kSatNullShift8 - kSatSqShift8)) - 1u);
        uint32_t SXo = SX, SXXo = SXX;
        // (opaque here: left alone, the compiler forms the f64 constants below in the header and carries twelve registers through every phase)
        asm volatile("" : "+s"(cS), "+s"(cSS), "+s"(rS), "+s"(rSS), "+s"(SXo), "+s"(SXXo));
        // T4 in closed form unless the window's own nulls are correlated anyway (wn): the never-written column / row take the chip's
        // last column / row out of n, sx, sxx -- its non-null pixels, with a chip that holds nulls
        const bool colT4 = !C::FULL && !wn && cx == csx - 2;
        const int rT4 = (C::FULL || wn) ? -1 : csy - 2 - ty0;            // tile row of the cells that reach the never-written last row
        const int Na = chip_nulls;
        const int cN = (int)(colQ >> kSatNullShift8), rN = (int)(rowQ >> kSatNullShift8), kN = corner == 0u ? 1 : 0;   // nulls of the chip's last column / row / corner pixel
        // (n, sx, sxx) of this lane's cells before the window's own nulls: off / on the T4 row
        const int n0 = NPX - Na - (colT4 ? CW - cN : 0), sx0 = (int)SXo - (colT4 ? (int)cS : 0), sxx0 = (int)SXXo - (colT4 ? (int)cSS : 0);
        const int n1 = n0 - (CW - rN) + (colT4 ? 1 - kN : 0), sx1 = sx0 - (int)rS + (colT4 ? (int)corner : 0), sxx1 = sxx0 - (int)rSS + (colT4 ? (int)(corner * corner) : 0);
        double dn0 = 0, dsx0 = 0, va0 = 0, dn1 = 0, dsx1 = 0, va1 = 0;
        if (!wn) {
            dn0 = (double)n0; dsx0 = (double)sx0; va0 = dn0 * (double)sxx0 - dsx0 * dsx0;
            dn1 = (double)n1; dsx1 = (double)sx1; va1 = dn1 * (double)sxx1 - dsx1 * dsx1;
        }
        auto cell_in = [&](int m, int i, double &dn, double &dsx, double &va, int &sxy, int &sy, int &syy) __attribute__((always_inline)) {
            const int ry = 16 * m + 4 * i + h;                  // (banded rows: band_row)
            sy = boxb[m][i]; syy = boxq[m][i];
            sxy = acc[m][i] + 128 * ((int)SXo + sy) - 16384 * NPX;          // (over all chip positions: a null is a zero factor)
            if (GEN && cn) {                                   // chip nulls take window pixels out of sy, syy
                sy -= ((-accy[m][i]) >> 7) + 128 * Na;
                syy -= accyl[m][i] + (128 + 256 * 128) * Na;
            }
            if (GEN && wn) {                                   // window nulls (T4 among them) take chip pixels out of n, sx, sxx
                const int nz = boxz[m][i];
                const int ca = ((-accz[m][i]) >> 7) + 128 * nz, caa = accl[m][i] + (128 + 256 * 128) * nz;
                dn = (double)(NPX - Na - nz + (cn ? (acczz[m][i] >> 14) : 0)); dsx = (double)((int)SXo - ca);
                va = dn * (double)((int)SXXo - caa) - dsx * dsx;
            } else {
                const bool rowT4 = ry == rT4;
                dn = rowT4 ? dn1 : dn0; dsx = rowT4 ? dsx1 : dsx0; va = rowT4 ? va1 : va0;
            }
        };
        // Iteration ci = 4 m + i finishes the band of tile rows 4 ci .. 4 ci + 3 of the wave's 16 columns.  REC: a climb reads no cell
        // outside the record's climb area (the scans are confined to it, best-of-pivots reads end positions of scans, the fit reads
        // visited cells), so the bands that miss its rows -- all eight in a wave whose columns miss it -- are left as the tile's bytes
        uint32_t bands = 0xffu;
        if constexpr (C::BOXT) bands = bands_t;
        else if constexpr (C::REC) {
            const uint32_t ar = area_w >> 8, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tix >> 6));
            const uint32_t x0 = ar & 31u, x1 = (ar >> 5) & 31u, y0 = (ar >> 10) & 31u, y1 = (ar >> 15) & 31u;
            bands = (w >= (x0 >> 4) && w <= (x1 >> 4)) ? ((2u << (y1 >> 2)) - (1u << (y0 >> 2))) & 0xffu : 0u;
        }
        uint32_t amb = 0u;
#pragma unroll
        for (int ci = 0; ci < 8; ci++) {
            if (C::REC && !((bands >> ci) & 1u)) continue;
            const int m = ci >> 2, i = ci & 3, ry = 16 * m + 4 * i + h;
            double dn, dsx, va; int sxy, sy, syy;
            cell_in(m, i, dn, dsx, va, sxy, sy, syy);
            const double dsy = (double)sy;
            const double num = dn * (double)sxy - dsx * dsy;
            const double P = va * (dn * (double)syy - dsy * dsy);
            bool redo;
            const double q = ncc_quot_fast(num, P, redo);
            if (redo) amb |= 1u << ci;
            val[ry * VP + sx_col] = (float)q;
            if constexpr (GEN) __builtin_amdgcn_sched_barrier(0);      // (general form: one cell at a time -- interleaved, the cells' f64 temporaries spill)
        }
        if (__any(amb != 0u)) {                            // rare (2^-15 of the cells): the reference's own operations
#pragma unroll
            for (int ci = 0; ci < 8; ci++) {
                if (!__any((amb >> ci) & 1u)) continue;        // (a skipped band has no bit)
                const int m = ci >> 2, i = ci & 3, ry = 16 * m + 4 * i + h;
                double dn, dsx, va; int sxy, sy, syy;
                cell_in(m, i, dn, dsx, va, sxy, sy, syy);
                const double dsy = (double)sy;
                const double num = dn * (double)sxy - dsx * dsy;
                const double den = ncc_den_exact(va * (dn * (double)syy - dsy * dsy));
                if ((amb >> ci) & 1u) val[ry * VP + sx_col] = ncc_quot_exact(num, den);
            }
        }
    }
    __syncthreads();
    MIMC3_MX_STAMP(3)
    if constexpr (C::SURF) {                                // the surface in k order (u outer): coalesced stores, LDS reads at stride VP
        const int S = 2 * p.full_R + 1, NC = S * S;
        float *sf = p.full_surf + (size_t)gidx * (size_t)NC;
        for (int k = (int)threadIdx.x; k < NC; k += NT) {
            const int x = k / S, y = k - S * x;
            sf[k] = val[y * VP + x];
        }
    }
    if (wave != 0) return;                                  // the sequential part needs one wave (lane k = pivot k)
    if constexpr (C::FULL) {
        full_tail<C>(p, val, gidx, lu, lv, lane);
        if constexpr (C::MULTI) {                           // (the record's lanes have left full_tail at different places: all 64 are back here)
            MIMC3_MX_STAMP(4)
            full_tail_multi<C>(p, val, gidx, lu, lv, lane);
            MIMC3_MX_STAMP(5)
            MIMC3_MX_STATS_OUT
        }
        return;
    }

    // ---- the climbs (lane k = pivot k) on the complete surface; trajectories as 4-bit codes per scan -------------------------
    auto inside = [&](int pu, int pvv) __attribute__((always_inline)) -> bool {     // the reference's boundary test (:703), true = scan allowed
        return !(pu - OCW <= 1 || pu + OCW >= Dx2 - 1 || pvv - OCW <= 1 || pvv + OCW >= Dy2 - 1);
    };
    // tile-relative cell of a scan centre
    auto relx = [&](int pu) __attribute__((always_inline)) -> int { return pu - OCW - tx0; };
    auto rely = [&](int pvv) __attribute__((always_inline)) -> int { return pvv - OCW - ty0; };
    constexpr int kSpecRounds = 16;
    int su, sv;
    {
        const int2 pv = reinterpret_cast<const int2 *>(smem + C::OFF_PIV)[lane];
        su = pv.x + dx2; sv = pv.y + dy2;
    }
    const int start_u = su, start_v = sv;
    // Lane k walks pivot k's climb on the complete surface, ignoring the visited state (which can only END a real climb earlier).  A scan's
    // move and running maximum depend on NCC values alone, with the reference's compare sequence (:736-741): recorded as move deltas, 4 bits
    // per scan ((du + 1) | (dv + 1) << 2; 5 = the scan did not move), plus one bit per scan "it raised the maximum".  Straight-line,
    // predicated: one wave-uniform loop, no divergent control flow (the compiler's exec-mask bookkeeping for a per-lane `while` was half
    // the loop's instructions).
    bool alive = lane < npiv && inside(su, sv);
    bool left = false;                                       // a scan would leave the tile (REC: the record's area)
    [[maybe_unused]] int axlo = 1, aylo = 1;
    [[maybe_unused]] uint32_t awx = 29u, awy = 29u;
    if constexpr (C::REC) mx_area_scan_bounds(area_w, axlo, awx, aylo, awy);
    uint32_t dlo = 0u, dhi = 0u, updm = 0u;
    int nsc = 0;
    float smax = -2.0f;                                      // the running maximum after all recorded scans (-2: no scan raised it)
    {
#pragma unroll 1
        for (int t = 0; t < kSpecRounds; t++) {
            if (!__any(alive)) break;
            const int rx = relx(su), ry = rely(sv);
            const bool in = C::REC ? ((unsigned)(rx - axlo) <= awx && (unsigned)(ry - aylo) <= awy) : ((unsigned)(rx - 1) <= 29u && (unsigned)(ry - 1) <= 29u);
            left = left || (alive && !in);
            const bool act = alive && in;
            const float *vp = val + (act ? ry : 1) * VP + (act ? rx : 1);          // (idle lanes read a harmless cell)
            float v[9];
#pragma unroll
            for (int j = 0; j < 9; j++) v[j] = vp[(j % 3 - 1) * VP + (j / 3 - 1)];
            const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(v[0], v[1]), v[2]), __builtin_fmaxf(__builtin_fmaxf(v[3], v[4]), v[5])),
                                            __builtin_fmaxf(__builtin_fmaxf(v[6], v[7]), v[8]));
            uint32_t mv = 8u;
#pragma unroll
            for (int j = 7; j >= 0; j--) mv = (v[j] == m) ? (uint32_t)j : mv;
            const bool up = act && (m > smax);
            smax = up ? m : smax;
            const bool moved = up && mv != 4u;
            const uint32_t q3 = (mv * 11u) >> 5;                                        // mv / 3 for 0..8
            const uint32_t d = moved ? (q3 | ((mv - 3u * q3) << 2)) : 5u;
            su += (int)(d & 3u) - 1; sv += (int)(d >> 2) - 1;
            const uint32_t dsh = act ? d << (4 * (t & 7)) : 0u;
            if (t < 8) dlo |= dsh; else dhi |= dsh;
            updm |= (up ? 1u : 0u) << t;
            nsc += act ? 1 : 0;
            alive = moved && inside(su, sv);
        }
    }
    if (__any(left)) { hand_on(kMxRest); return; }
    MIMC3_MX_STAMP(4)

    // ---- exact replay: the visited state only decides HOW MANY scans of a pivot really happen (newncc != 0, :699) -- sequential over
    //      pivots; lane r holds the visited bits of tile row r (match_px_kernel.hip, "exact replay", with 32-bit rows)
    uint32_t tp = 0u;                                        // lane k: pivot k's scans performed | the tile-relative cell it ended on << 8 (x), << 16 (y)
    uint32_t vrow = 0u;
    const uint32_t head = (uint32_t)(relx(start_u) & 0xff) | ((uint32_t)(rely(start_v) & 0xff) << 8) | ((uint32_t)nsc << 16);
    auto replay_pivot = [&](int kk) __attribute__((always_inline)) -> uint32_t {
        const uint32_t hd = (uint32_t)__builtin_amdgcn_readlane((int)head, kk);
        const int n_k = (int)(hd >> 16);
        int ccx = (int)(hd & 0xffu), cy1 = (int)((hd >> 8) & 0xffu) - 1;      // centre column, centre row - 1 (tile-relative)
        unsigned long long cur = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)dhi, kk) << 32) |
                                 (uint32_t)__builtin_amdgcn_readlane((int)dlo, kk);
        int t = 0;
        while (t < n_k) {
            // rows cy1 .. cy1 + 2 (= lanes) test and set their three bits; fresh3 = the lanes that held an unvisited one
            unsigned long long fresh3, sv2;
            uint32_t tmp;
            const uint32_t m3 = 7u << (ccx - 1);
            asm volatile("v_subrev_u32_e32 %[tmp], %[y], %[l1]\n\t"
                         "v_cmp_gt_u32_e32 vcc, 3, %[tmp]\n\t"
                         "s_and_saveexec_b64 %[sv], vcc\n\t"
                         "v_bitop3_b32 %[tmp], %[m], %[v], %[m] bitop3:0x30\n\t"      // m3 & ~vrow
                         "v_cmp_ne_u32_e32 vcc, 0, %[tmp]\n\t"
                         "v_or_b32_e32 %[v], %[m], %[v]\n\t"
                         "s_mov_b64 exec, %[sv]\n\t"
                         "s_mov_b64 %[fr], vcc"
                         : [tmp] "=&v"(tmp), [sv] "=&s"(sv2), [fr] "=s"(fresh3), [v] "+v"(vrow)
                         : [y] "s"(cy1), [l1] "v"(lane), [m] "s"(m3)
                         : "vcc", "scc");
            t++;
            const uint32_t d = (uint32_t)cur & 15u;
            cur >>= 4;
            ccx += (int)(d & 3u) - 1; cy1 += (int)(d >> 2) - 1;
            if (fresh3 == 0ull) break;
            if (d == 5u) break;
        }
        // (the loop has stepped the centre past the t scans performed: where the pivot ended -- kept with t, so no lane decodes its codes again)
        return (uint32_t)t | ((uint32_t)ccx & 0xffu) << 8 | ((uint32_t)(cy1 + 1) & 0xffu) << 16;
    };
    // ---- the shortcut: only three things are read behind the replay -- the pivot that wins best-of-pivots with its end cell and maximum,
    //      the visited bits of the fit's nine cells, and T of a lane still alive at the cap.  With no lane alive and M* = max M_k > -2
    //      (M_k = lane k's smax: pivot k's maximum if its real climb performed every recorded scan), let w be the first pivot with
    //      M_w = M*.  Every real climb is a prefix of the recorded one, so the cells visited before pivot w are a subset of U, the 3 x 3
    //      neighbourhoods of all recorded scans of the pivots before w; a smaller visited set cannot end a climb sooner.  So if w, replayed
    //      alone from U, performs all its scans and its last one did not move, its real climb does too: it ends on the same cell with M*,
    //      no earlier pivot reaches M* and no later one exceeds it (strict >, :747), and that last scan visited the fit's nine cells.
    //      Otherwise the full replay runs from an empty visited set, as without the shortcut.  
    int px = relx(dx2), py = rely(dy2);                      // the peak as a tile-relative cell
    float best = -2.0f;
    bool shortcut = false;
    uint32_t outcome = kReplayNoPre;
    if (p.replay_shortcut && !__any(alive)) {
        float bv = smax;                                     // (a lane without a pivot never scanned: -2)
        int bi = lane;
        argmax_row16(bv, bi);
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        bv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bv)));
        const int w = __builtin_amdgcn_readfirstlane(bi) & 63;
        if (bv > -2.0f) {
            const unsigned long long before = __ballot(nsc > 0) & ((1ull << w) - 1ull);      // the pivots in front of w that scan at all
            if (before != 0ull) {                            // U: those lanes walk their deltas again, three row masks per scan
                if (lane < 32) vis[lane] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (lane < w) {
                    int cx = relx(start_u), cy = rely(start_v);
                    unsigned long long cur = ((unsigned long long)dhi << 32) | dlo;
                    for (int t = 0; t < nsc; t++) {          // (every recorded scan lies inside the tile: cx, cy in 1 .. 30)
                        const uint32_t m3 = 7u << (cx - 1);
                        atomicOr(&vis[cy - 1], m3); atomicOr(&vis[cy], m3); atomicOr(&vis[cy + 1], m3);
                        const uint32_t d = (uint32_t)cur & 15u;
                        cur >>= 4;
                        cx += (int)(d & 3u) - 1; cy += (int)(d >> 2) - 1;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                vrow = vis[lane & 31];
            }
            const uint32_t tpw = replay_pivot(w);
            const int n_w = __builtin_amdgcn_readlane(nsc, w);
            const uint32_t lastw = (uint32_t)__builtin_amdgcn_readlane((int)(n_w > 8 ? dhi : dlo), w);
            shortcut = (int)(tpw & 0xffu) == n_w && ((lastw >> (4 * ((n_w - 1) & 7))) & 15u) == 5u;
            if (shortcut) { px = (int)((tpw >> 8) & 0xffu); py = (int)(tpw >> 16); best = bv; }
            else vrow = 0u;
            outcome = shortcut ? (before != 0ull ? kReplayShortU : kReplayShort) : kReplayFellBack;
        }
    }
    if (p.stats && lane == 0) p.stats[kStatW * (size_t)blockIdx.x + 8] = outcome + 1ull;
    if (!shortcut) {
        for (int kk = 0; kk < npiv; kk++) {
            const uint32_t tpk = replay_pivot(kk);
            tp = (lane == kk) ? tpk : tp;
        }
        const int T = (int)(tp & 0xffu);
        // a pivot whose speculation was cut at 16 scans and whose real climb consumed all of them: the register-tiled kernel decides
        if (__any(alive && T == nsc)) { hand_on(kMxRest); return; }
    }
    if (lane < 32) vis[lane] = vrow;
    MIMC3_MX_STAMP(5)

    // ---- best of pivots (:744-752): after its last updating scan a pivot sits on the arg-max cell
    if (!shortcut) {
        const int T = (int)(tp & 0xffu);
        const int fx = (int)((tp >> 8) & 0xffu), fy = (int)(tp >> 16);           // (a pivot without a scan: not read)
        const bool upd = (updm & ((T >= 32 ? 0u : (1u << T)) - 1u)) != 0u;      // some scan among the T performed raised the maximum
        const float fmax = upd ? val[fy * VP + fx] : -2.0f;
        float bv = (lane < npiv) ? fmax : -__builtin_inff();
        int bi = lane;
        argmax_row16(bv, bi);
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        bv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bv)));
        bi = __builtin_amdgcn_readfirstlane(bi);
        if (bv > -2.0f) {                                    // strict >, first pivot attaining the maximum wins
            const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)tp, bi & 63);
            px = (int)((pk >> 8) & 0xffu); py = (int)(pk >> 16); best = bv;
        }
    }
    __builtin_amdgcn_wave_barrier();                          // (one wave: its LDS operations are performed in order)
    // ---- 3x3 quadratic fit (:757-788), the reference's arithmetic value by value (match_px_kernel.hip) ------------------------------
    // the nine cells: lane 3 r + c loads cell (px - 1 + c, py - 1 + r) and its visited bit -- clamped addresses and a select, no branch --
    // and the values reach the fit's lanes by readlane
    float n9[9];
    {
        const int j = lane < 9 ? lane : 0, r = (j * 11) >> 5, c = j - 3 * r;
        const int x = px - 1 + c, y = py - 1 + r;
        const bool in = (unsigned)x < 32u && (unsigned)y < 32u;                                  // (a cell outside the tile was never scanned)
        const int xc = in ? x : 0, yc = in ? y : 0;
        const uint32_t seen = (vis[yc] >> xc) & 1u;
        const float cv = val[yc * VP + xc];
        const float nv = (in && seen != 0u) ? cv : -2.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) n9[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nv), k));
    }
    if (lane < 5) {
        const float e0 = 6 * n9[0] - 12 * n9[1] + 6 * n9[2] + 6 * n9[3] - 12 * n9[4] + 6 * n9[5] + 6 * n9[6] - 12 * n9[7] + 6 * n9[8];
        const float e1 = 9 * n9[0] - 9 * n9[2] - 9 * n9[6] + 9 * n9[8];
        const float e2 = 6 * n9[0] + 6 * n9[1] + 6 * n9[2] - 12 * n9[3] - 12 * n9[4] - 12 * n9[5] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
        const float e3 = -6 * n9[0] + 6 * n9[2] - 6 * n9[3] + 6 * n9[5] - 6 * n9[6] + 6 * n9[8];
        const float e4 = -6 * n9[0] - 6 * n9[1] - 6 * n9[2] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
        double cp = (double)(lane == 0 ? e0 : (lane == 1 ? e1 : (lane == 2 ? e2 : (lane == 3 ? e3 : e4))));
        cp /= 36;
        auto from_lane = [&](int ln) __attribute__((always_inline)) -> double {
            const long long bits = __double_as_longlong(cp);
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, ln), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), ln);
            return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        };
        const double cp0 = from_lane(0), cp1 = from_lane(1), cp2 = from_lane(2), cp3 = from_lane(3), cp4 = from_lane(4);
        const float num = lane == 0 ? (float)(-2 * cp2 * cp3 + cp1 * cp4) : (float)(-2 * cp0 * cp4 + cp1 * cp3);
        const double det = 4 * cp0 * cp2 - cp1 * cp1;
        float o = (float)((double)num / det);
        o += (float)(lane == 0 ? px + OCW + tx0 - dx2 : py + OCW + ty0 - dy2);
        if (lane < 2) p.out[3 * (size_t)gidx + lane] = o;
        if (lane == 0) p.out[3 * (size_t)gidx + 2] = best;
    }
    if constexpr (C::REC) {
        if (adv) {             // finished: the register-tiled launch leaves at this bit of the record's `tile` dword, right behind its header load
            if (lane == 0) {
                reinterpret_cast<uint32_t *>(p.rest_recs + rpos)[8] = tile_w | kRecDone;
                if (p.stats) p.stats[kStatW * (size_t)blockIdx.x + 7] = 2ull;
            }
            return;            // ("clean: N points staged" counts the clean list's workgroups alone)
        }
    }
    MIMC3_MX_STAMP(6)
    MIMC3_MX_STATS_OUT
}

template <class C>
static hipError_t launch_one(MatchU8Args a, hipStream_t stream)
{
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    static unsigned long long *d_stats = nullptr;
    static const bool want_stats = getenv("MIMC3_MX_STATS") != nullptr;
    static size_t stats_n = 0;
    static std::mutex stats_mu;                      // diagnostics only
    std::unique_lock<std::mutex> stats_lock(stats_mu, std::defer_lock);
    if (want_stats) {
        stats_lock.lock();
        if (stats_n < (size_t)nb) {
            if (d_stats) (void)hipFree(d_stats);
            (void)hipMalloc(&d_stats, kStatW * sizeof(unsigned long long) * (size_t)nb);
            stats_n = nb;
        }
        (void)hipMemsetAsync(d_stats, 0, kStatW * sizeof(unsigned long long) * (size_t)nb, stream);
    }
    a.stats = want_stats ? d_stats : nullptr;
    hipLaunchKernelGGL(match_ncc_dlc_mx<C>, dim3(nb), dim3(C::NT), 0, stream, a);
    if (want_stats) {
        (void)hipStreamSynchronize(stream);
        unsigned long long *hh = (unsigned long long *)malloc(kStatW * sizeof(unsigned long long) * (size_t)nb);
        (void)hipMemcpy(hh, d_stats, kStatW * sizeof(unsigned long long) * (size_t)nb, hipMemcpyDeviceToHost);
        unsigned long long hsum[kStatW] = {0};
        size_t live = 0;
        size_t adv_tried = 0, adv_done = 0;              // (slot 7: an advance-list workgroup's 1 = tried, 2 = finished; it writes no phase clocks)
        size_t rs[4] = {0, 0, 0, 0};                     // (slot 8: the replay shortcut's outcome + 1 of a workgroup that reached the replay)
        for (size_t b = 0; b < (size_t)nb; b++) {
            if (hh[kStatW * b]) live++;
            for (int i = 0; i < 7; i++) hsum[i] += hh[kStatW * b + i];
            adv_tried += hh[kStatW * b + 7] != 0; adv_done += hh[kStatW * b + 7] == 2;
            if (hh[kStatW * b + 8]) rs[(hh[kStatW * b + 8] - 1) & 3]++;
        }
        free(hh);
        const double d = live ? (double)live : 1.0;
        int32_t nn = 0, nr = 0;
        {
            unsigned char *hf = (unsigned char *)malloc((size_t)a.N);
            (void)hipMemcpy(hf, a.mx_flags, (size_t)a.N, hipMemcpyDeviceToHost);
            for (int i = 0; i < a.N; i++) { nn += hf[i] == kMxNulls; nr += hf[i] == kMxRest; }
            free(hf);
        }
        fprintf(stderr, "[mimc3 mx stats] ocw %d %s: %zu points staged; cycles/point: stage %.0f products %.0f box sums %.0f ncc %.0f climb %.0f replay %.0f fit %.0f; lists so far: nulls %d rest %d\n",
                C::OCW, C::GEN ? (C::CN ? "general" : "window nulls") : "clean", live, hsum[0] / d, hsum[1] / d, hsum[2] / d, hsum[3] / d, hsum[4] / d, hsum[5] / d, hsum[6] / d, nn, nr);
        if (!C::FULL && !C::GEN && a.mx_classified && a.point_count) {      // (without records the list is empty and no workgroup tries)
            int32_t nadv = 0;
            (void)hipMemcpy(&nadv, a.point_count + 2, sizeof(nadv), hipMemcpyDeviceToHost);
            fprintf(stderr, "[mimc3 mx stats] advance: list %d tried %zu finished %zu\n", nadv, adv_tried, adv_done);
        }
        if (!C::FULL)
            fprintf(stderr, "[mimc3 mx stats] replay shortcut: taken with U empty %zu, taken with U built %zu, fell back %zu, preconditions failed %zu\n",
                    rs[kReplayShort], rs[kReplayShortU], rs[kReplayFellBack], rs[kReplayNoPre]);
    }
    return hipGetLastError();
}

// diagnostics (MIMC3_MX_STATS): the classes and list lengths as u8_classify left them, before any matcher launch touches them
static hipError_t classify_stats(const MatchU8Args &a, const int32_t *lists, hipStream_t stream)
{
    static const bool want_stats = getenv("MIMC3_MX_STATS") != nullptr;
    if (!want_stats) return hipSuccess;
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    unsigned char *hf = (unsigned char *)malloc((size_t)a.N);
    int32_t head[2] = {0, 0};
    (void)hipMemcpy(hf, a.mx_flags, (size_t)a.N, hipMemcpyDeviceToHost);
    (void)hipMemcpy(head, lists, sizeof(head), hipMemcpyDeviceToHost);
    int n[4] = {0, 0, 0, 0};
    for (int i = 0; i < a.N; i++) n[hf[i] & 3]++;
    free(hf);
    fprintf(stderr, "[mimc3 mx stats] u8_classify: classes clean %d rest %d nulls %d window-nulls %d; lists clean %d rest %d\n", n[0], n[kMxRest],
            n[kMxNulls], n[kMxWn], head[0], head[1]);
    return hipSuccess;
}

}  // namespace mx

bool match_mx_supported(int ocw, int max_npiv, int win_half, int max_abs_u, int max_abs_v)
{
    static const int off = getenv("MIMC3_MX") ? atoi(getenv("MIMC3_MX")) : 1;      // tuning / A-B: 0 = never take this kernel
    if (!off) return false;
    if (win_half > 0) return false;                   // full-square search areas (control-point stage): many pivots, not this kernel
    // A point whose pivots (with the ring of cells their first scans touch) do not fit the 32 x 32 tile is flagged for the
    // register-tiled kernel by the kernel itself, point by point: a velocity field with a few fast points keeps its slow ones here.
    // (A launch whose every corridor is too long -- BASELINE C4: 31 pivots -- only passes through: u8_classify puts every point on the
    // rest list and this kernel's workgroups leave after one scalar load.)  The launch's maxima still size the register-tiled kernel's
    // LDS carve, as without this kernel.
    (void)max_abs_u; (void)max_abs_v;
    if (max_npiv > 64) return false;                  // (the many-pivot kernel forms: no tables)
    return ocw == 7 || ocw == 15 || ocw == 16 || ocw == 30 || ocw == 32 || ocw == 40;
}

template <bool GEN, bool CN>
static hipError_t launch_form(const MatchU8Args &a, hipStream_t stream)
{
    switch (a.ocw) {
    case 7: return mx::launch_one<mx::Cfg<7, GEN, CN>>(a, stream);
    case 15: return mx::launch_one<mx::Cfg<15, GEN, CN>>(a, stream);
    case 16: return mx::launch_one<mx::Cfg<16, GEN, CN>>(a, stream);
    case 30: return mx::launch_one<mx::Cfg<30, GEN, CN>>(a, stream);
    case 32: return mx::launch_one<mx::Cfg<32, GEN, CN>>(a, stream);
    case 40: return mx::launch_one<mx::Cfg<40, GEN, CN>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

template <bool BOXT>
static hipError_t launch_rec_form(const MatchU8Args &a, hipStream_t stream)
{
    switch (a.ocw) {
    case 7: return mx::launch_one<mx::RecCfg<7, BOXT>>(a, stream);
    case 15: return mx::launch_one<mx::RecCfg<15, BOXT>>(a, stream);
    case 16: return mx::launch_one<mx::RecCfg<16, BOXT>>(a, stream);
    case 30: return mx::launch_one<mx::RecCfg<30, BOXT>>(a, stream);
    case 32: return mx::launch_one<mx::RecCfg<32, BOXT>>(a, stream);
    case 40: return mx::launch_one<mx::RecCfg<40, BOXT>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

bool mx_box_table_on()
{
    // tuning / A-B: 0 = the record forms compute the window-side box sums by MFMA, as the other forms do
    static const int on = getenv("MIMC3_MX_BOX_TABLE") ? atoi(getenv("MIMC3_MX_BOX_TABLE")) : 1;
    return on != 0;
}

bool u8_advance_on()
{
    // tuning / A-B: 0 = no advance list (every window-null point waits for the register-tiled launch); needs the point records
    static const int on = getenv("MIMC3_U8_ADVANCE") ? atoi(getenv("MIMC3_U8_ADVANCE")) : 1;
    return on != 0 && u8_point_records_on();
}

bool mx_area_on()
{
    // tuning / A-B: 0 = a clean point's area is the whole tile (every band finished, only a climb that leaves the tile handed on)
    static const int on = getenv("MIMC3_MX_AREA") ? atoi(getenv("MIMC3_MX_AREA")) : 1;
    return on != 0 && u8_advance_on();
}

bool u8_point_records_on()
{
    static const int on = getenv("MIMC3_U8_RECS") ? atoi(getenv("MIMC3_U8_RECS")) : 1;      // tuning / A-B: 0 = the headers read memory, as without records
    return on != 0;
}

// u8_classify, then up to three launches: the clean form over the clean list, then the forms for the other classes in flag mode.  Points
// none takes are on the rest list afterwards (and carry kMxRest in mx_flags).
hipError_t launch_match_mx(MatchU8Args a, int32_t *lists, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.mx_flags || !a.sat0 || !a.sat1 || !lists || !a.ovf_count) return hipErrorInvalidValue;
    // Which null-ridden points stay on the matrix cores: none by default.  Both forms for them are built, tested and bit-identical at
    // every chip size, but measured at BASELINE C2 (ns per point; the register-tiled kernel's sparse corrections: 18 at ocw 16, 66 at
    // ocw 40) the window-null form (null-free chip: four correlations) costs 16 and leaves that kernel the chip-null points alone, which
    // it then runs at 23.5 -- 2.84 ms per pass against 2.75; the general form (chip nulls too: eight correlations) costs 19 at ocw 16
    // and 86 at ocw 40, its operand planes leaving two to three workgroups per CU.  The clean form takes the points without nulls
    // (8.9 ns against 11.3, 40 against 66 at ocw 40).  MIMC3_MX_WN / MIMC3_MX_GEN = 1 turn the other two on.
    static const int wn_env = getenv("MIMC3_MX_WN") ? atoi(getenv("MIMC3_MX_WN")) : 0;
    static const int gen_env = getenv("MIMC3_MX_GEN") ? atoi(getenv("MIMC3_MX_GEN")) : 0;
    a.mx_wn_on = wn_env > 0 ? 1 : 0;
    a.mx_gen_on = gen_env != 0 ? 1 : 0;
    a.mx_classified = 1;
    a.replay_shortcut = replay_shortcut_on() ? 1 : 0;
    a.point_flags = nullptr;
    a.point_count = lists; a.point_list = lists + kU8ListHead;
    a.rest_count = lists + 1; a.rest_list = lists + kU8ListHead + (size_t)a.N;
    // with point records (U8PointRec): the classifier leaves every listed point's header at its list position, the clean form reads it
    // there, and a point it hands on takes its record along to the rest list
    a.point_recs = nullptr; a.rest_recs = nullptr;
    if (u8_point_records_on()) { a.point_recs = u8_list_recs(lists, a.N); a.rest_recs = u8_list_recs(lists, a.N) + (size_t)a.N; }
    hipError_t e = launch_u8_classify(a, lists, u8_advance_on(), mx_area_on(), stream);
    if (e == hipSuccess) e = mx::classify_stats(a, lists, stream);
    if (e == hipSuccess) e = a.point_recs ? (mx_box_table_on() ? launch_rec_form<true>(a, stream) : launch_rec_form<false>(a, stream)) : launch_form<false, false>(a, stream);
    a.point_list = nullptr; a.point_count = nullptr; a.point_recs = nullptr;
    a.point_flags = a.mx_flags;
    if (e == hipSuccess && a.mx_wn_on) { a.flag_value = kMxWn; e = launch_form<true, false>(a, stream); }
    if (e == hipSuccess && a.mx_gen_on) { a.flag_value = kMxNulls; e = launch_form<true, true>(a, stream); }
    return e;
}

// Exhaustive search: every point on the matrix cores.  The clean form runs over all points and flags the null-ridden ones for the
// window-null form (nulls in the search box only) or the general form (chip nulls too), which run right behind in flag mode.
// (FC: FullCfg, FullPeakCfg when the caller wants the arg-max cells, or FullMultiCfg when it wants the candidates; FullSurfCfg /
//  FullMultiSurfCfg when it wants the surfaces as well)
template <template <int, bool, bool> class FC, bool GEN, bool CN>
static hipError_t launch_full_form(const MatchU8Args &a, hipStream_t stream)
{
    switch (a.ocw) {
    case 7: return mx::launch_one<FC<7, GEN, CN>>(a, stream);
    case 15: return mx::launch_one<FC<15, GEN, CN>>(a, stream);
    case 16: return mx::launch_one<FC<16, GEN, CN>>(a, stream);
    case 30: return mx::launch_one<FC<30, GEN, CN>>(a, stream);
    case 32: return mx::launch_one<FC<32, GEN, CN>>(a, stream);
    case 40: return mx::launch_one<FC<40, GEN, CN>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

template <template <int, bool, bool> class FC>
static hipError_t launch_full_forms(MatchU8Args a, hipStream_t stream)
{
    hipError_t e = launch_full_form<FC, false, false>(a, stream);
    a.point_flags = a.mx_flags;
    if (e == hipSuccess) { a.flag_value = kMxWn; e = launch_full_form<FC, true, false>(a, stream); }
    if (e == hipSuccess) { a.flag_value = kMxNulls; e = launch_full_form<FC, true, true>(a, stream); }
    return e;
}

hipError_t launch_match_full_mx(MatchU8Args a, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.mx_flags || !a.sat0 || !a.sat1 || a.full_R < 1 || a.full_R > 15) return hipErrorInvalidValue;
    a.mx_wn_on = 1; a.mx_gen_on = 1; a.mx_classified = 0;
    a.point_list = nullptr; a.point_count = nullptr; a.point_flags = nullptr; a.point_recs = nullptr; a.rest_recs = nullptr;
    if (a.full_surf && a.full_peak) return hipErrorInvalidValue;
    if (a.full_cand) {
        if (a.full_peak || a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks) return hipErrorInvalidValue;
        return a.full_surf ? launch_full_forms<mx::FullMultiSurfCfg>(a, stream) : launch_full_forms<mx::FullMultiCfg>(a, stream);
    }
    if (a.full_surf) return launch_full_forms<mx::FullSurfCfg>(a, stream);
    return a.full_peak ? launch_full_forms<mx::FullPeakCfg>(a, stream) : launch_full_forms<mx::FullCfg>(a, stream);
}

}  // namespace mimc3
