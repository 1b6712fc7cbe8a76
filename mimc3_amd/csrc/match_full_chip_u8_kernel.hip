// match_full_chip_u8_kernel.hip -- exhaustive-search NCC offsets for gfx950 on 8-BIT pairs at ANY chip half-width 1 <= ocw <= 80, on the
// matrix cores (mimc3_match_ncc_full_chip_class).  ocw is a RUN-TIME value here.
//
// It is the exhaustive-search (FULL) half of match_ncc_dlc_mx (match_mx_kernel.hip, which has the derivation) with the chip size taken
// out of the template: the Toeplitz-band GEMM on v_mfma_i32_16x16x64_i8 over the 32 x 32 cell tile whose origin is c - R, x ^ 0x80 at
// staging, two waves per point (wave w owns the cell columns [16 w, 16 w + 16) x 32 rows), the window-side box sums on the matrix pipe
// against two bands of ones, the finish and the tails of match_full_tail.h as they stand (ncc_quot_fast with its guard and the exact
// redo, full_tail, full_tail_multi), the surface in LDS at pitch 33.  No climb, no point records, no T4 terms.
//   run time   the chip row length (CW, CD, LASTN, the chip plane pitch CP), the tile pitch PW, the 16-row tile and K-chunk counts of the
//              box sums (NTR, KCV) and the trip count of the double-buffered row loop (CWE = CW + 1: the zero row behind the odd chip)
//              come from chip_u8_layout(ocw), the one expression the kernel, the launch and the static checks share.  The layout does
//              not depend on R (the tile is 32 x 32 cells whatever the radius) nor on the form (one chip plane in both, see below).
//   template   KCW, the K chunks (64 window columns) per chip row and cell tile: 1 (ocw <= 24), 2 (ocw <= 56) or 3.  It sizes the operand
//              registers of the row loop, so it stays a template parameter; the launch picks the instantiation from the layout.
//   bands      the two bands of ones are formed from the lane index (hb once per workgroup, vb per use): no tables.
//   tables     the packed u8 table (sat_kernel.h) is exact for one query only up to 8,224 pixels, so the chip's sum, sum of squares and null
//              count are ALWAYS taken as sub-boxes of at most 64 x 64 pixels, one per lane, the three fields added apart (chip_sums_u8):
//              from CW = 91 (ocw 45) on one query would carry between the fields on near-saturated data.  The box's null count comes
//              from sat_nulls_u8, which cuts in the same way.
// Two forms.  The clean form runs over all points, classifies each one at staging from the table queries and sets the class byte of a
// point that holds a null in its chip or its search box (kMxNulls in mx_flags); the masked form runs right behind it in flag mode and
// takes any null pattern.  A null is the pixel 0: sum ab needs no mask; the other five sums are the clean ones minus correlations with
// the null indicators zb = [b == 0], za = [a == 0] on the same pipe --
//   sum zb (box sums), sum a zb, sum a^2 zb (a^2 as two byte planes)  take chip pixels out of n, sx, sxx under window nulls,
//   sum b za, sum b^2 za (b^2 as two byte planes), sum za zb          take window pixels out of sy, syy (and put back what n lost twice)
// -- with every extra operand formed IN REGISTERS from the two that are staged anyway: zb and the planes of b^2 from the tile row, za and
// the planes of a^2 from the Toeplitz row (masked by the band of chip bytes: its padding is not a pixel).  So the masked form stages
// the one chip plane of the clean form and fits LDS whole at every chip size; it is not banded.
// Integer bounds (CW <= 161, pixels <= 255; asserted below): the largest true sum is 161^2 255^2 = 1,685,513,025 < 2^31; in offset form
// |sum a'b'| <= 161^2 128^2 < 2^29, and every correlation with a null plane (-128 per null) is bounded by the same product; a row-box sum
// of b^2 is < 2^24 (three byte planes), one of b < 2^16 (two), a row's null count <= 161 (one plane in offset form).  sum ab itself is
// put together in f64 (exact): sum a'b' + 128 (sx + sy) comes within 1.5 % of 2^31 before 128^2 CW^2 is taken off.
// On an 8-bit pair every sum of the float kernel (match_full_chip_kernel.hip) is the same exact integer, its finish the reference's own
// operations and this one's the guarded fast form of them: record, candidates and surface are that kernel's bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "sat_kernel.h"
#include "match_full_tail.h"
#include "stack_acc.h"

namespace mimc3 {

namespace fchip8 {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef unsigned long long SatT;

constexpr int kNT = 128;                            // two wave64 per grid point
constexpr int kVP = 33;                             // pitch (words) of the NCC surface
constexpr int kValBytes = 4 * 32 * kVP;
constexpr int kCH0 = 16;                            // leading zeros of the chip plane (row 0's left padding)

static_assert(kFullChipMaxOcw == 80, "the bounds below are those of CW = 161");
static_assert(161ll * 161 * 255 * 255 < (1ll << 31), "the largest true sum fits an i32");
static_assert(161ll * 161 * 128 * 128 < (1ll << 29), "offset form: sum a'b', and every correlation with a null plane");
static_assert(161ll * 255 * 255 < (1ll << 24) && 161 * 255 < (1 << 16), "row-box sums: three byte planes of b^2, two of b");
static_assert(64ll * 64 * 255 < (1ll << kSatSqShift8) && 64ll * 64 * 255 * 255 < (1ll << (kSatNullShift8 - kSatSqShift8)) && 64 * 64 < (1 << (64 - kSatNullShift8)),
              "a 64 x 64 sub-box fits every field of the packed table");

struct Layout {
    int CW, KW, KCW, SW, PW, NTR, KCV, CD, LASTN, CP, CWE, CHB, off_ch, lds;
};

// the one expression of the layout (match_mx_kernel.hip's Cfg, as a function of a run-time ocw)
__host__ __device__ constexpr Layout chip_u8_layout(int ocw)
{
    Layout l{};
    l.CW = 2 * ocw + 1;
    l.KW = l.CW + 31;                               // window columns (and rows) the 32 x 32 cells of a tile reach
    l.KCW = (l.CW + 15 + 63) / 64;                  // MFMAs per chip row and 16 x 16 cell tile
    const int RDW = 16 + 64 * l.KCW;                // bytes of a tile row some wave reads
    l.SW = (l.KW + 15) & ~15;                       // bytes of a tile row that are staged
    const int PW0 = RDW > l.SW ? RDW : l.SW;
    l.PW = ((PW0 / 16) & 1) ? PW0 : PW0 + 16;       // pitch 16 x odd
    l.NTR = (l.KW + 15) / 16;                       // 16-row tiles of the row-box sums
    l.KCV = (l.NTR + 3) / 4;                        // K chunks (64 tile rows) of the vertical sums
    l.CD = (l.CW + 3) / 4;                          // dwords per chip row
    l.LASTN = l.CW - 4 * (l.CD - 1);                // valid bytes of a chip row's last dword
    const int CP0 = (l.CW + 15 + 3) & ~3;
    l.CP = CP0 > 64 * l.KCW ? CP0 : 64 * l.KCW;     // chip plane pitch: a row's right padding is the next row's left padding
    l.CWE = l.CW + 1;                               // chip rows the product loop walks, two per trip: the all-zero row behind the odd chip
    l.CHB = (kCH0 + l.CWE * l.CP + 16 + 15) & ~15;  // the chip plane (+ the read-ahead of the last row's last lane)
    const int ldsw = (16 * l.NTR + 1) * l.PW;       // the tile (+ the row the product loop's zero chip row reads)
    l.off_ch = ((ldsw > kValBytes ? ldsw : kValBytes) + 15) & ~15;      // the surface reuses the tile's bytes
    l.lds = l.off_ch + l.CHB;
    return l;
}

// the most 16-row tiles of the box sums in a KCW class (KW <= 64 KCW + 16, and 192 at the largest chip): what the box-sum loops are unrolled to
__host__ __device__ constexpr int max_ntr(int kcw) { return kcw >= 3 ? 12 : (64 * kcw + 16 + 15) / 16; }

constexpr bool layouts_fit()
{
    for (int ocw = 1; ocw <= kFullChipMaxOcw; ocw++) {
        const Layout l = chip_u8_layout(ocw);
        if (l.KCW < 1 || l.KCW > 3 || l.NTR > 12 || l.KCV > 3 || l.lds > 160 * 1024) return false;
        if (l.KW > 16 * l.NTR || l.SW > l.PW || 16 + 64 * l.KCW > l.PW || l.CP < l.CW + 15 || l.CP < 64 * l.KCW) return false;
        if (l.LASTN < 1 || l.LASTN > 4 || 4 * l.CD > l.CP) return false;
        if ((l.KCW == 1) != (ocw <= 24) || (l.KCW == 3) != (ocw >= 57)) return false;      // (what the occupancy targets below assume)
        if (l.NTR > max_ntr(l.KCW)) return false;
    }
    return true;
}
static_assert(layouts_fit(), "every ocw fits its LDS, and the reads stay inside the rows and planes of the layout");
static_assert(2 * chip_u8_layout(kFullChipMaxOcw).lds <= 160 * 1024, "two workgroups per CU at the largest chip");

template <int KCW_, bool GEN_, bool MULTI_, bool SURF_>
struct Cfg {                                        // (VP, PEAK, MULTI: what match_full_tail.h asks of a configuration)
    static constexpr int KCW = KCW_, VP = kVP;
    static constexpr bool GEN = GEN_, PEAK = false, MULTI = MULTI_, SURF = SURF_;
    // occupancy target, waves per SIMD: the most that leaves the kernel without scratch (at 6 the clean form of the small chips spills,
    // at 4 the masked one), never above what LDS admits at the smallest chip of the class anyway (16, 7, 2 workgroups per CU)
    static constexpr int MINW = KCW_ == 1 ? (GEN_ ? 3 : 5) : KCW_ == 2 ? (GEN_ ? 2 : 3) : 1;
    static constexpr bool ACC = false;              // (the accumulating forms: AccCfg below)
};
// The accumulating (ACC) forms, a third output beside the record and SURF forms: the finished surface is added into the stack where
// the SURF form stores it (stack_acc.h) and no tail runs -- no record, candidate or surface is written.  Configurations of their own, so
// that the names, registers and code of every Cfg instantiation stay what they were; the occupancy targets are the record forms'
// (the accumulation runs after the cell registers are dead: no scratch at any of them, tools/kres.py)
template <int KCW_, bool GEN_>
struct AccCfg : Cfg<KCW_, GEN_, false, false> {
    static constexpr bool ACC = true;
};
// The PEAK forms, the record-only forms that also leave every point's arg-max cell k = (su + R)(2R + 1) + (sv + R), or -1 without one, in
// full_peak, where a pyramid's next level takes its search centre from (mimc3_match_ncc_pyramid_chip; FullPeakCfg of match_mx_kernel.hip).
// Configurations of their own, as AccCfg: the occupancy targets are the record forms'.  Every point gets exactly one store per search:
// the clean form writes -1 with the NaN record (a chip outside the level, a box beyond the border) and the cell of a point it finishes,
// and hands a flagged point over untouched; the masked form writes -1 with its -3 and the cell of a point it finishes
template <int KCW_, bool GEN_>
struct PeakCfg : Cfg<KCW_, GEN_, false, false> {
    static constexpr bool PEAK = true;
};

__device__ __forceinline__ uint32_t alignb(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_alignbyte(hi, lo, s); }
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
__device__ __forceinline__ v4i mfma(const v4i &a, const v4i &b, const v4i &c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }

// the squares of the four pixels of a dword as the two byte planes (x^2 & 255, x^2 >> 8)
__device__ __forceinline__ void squares_dword(uint32_t x, uint32_t &lo, uint32_t &hi)
{
    const uint32_t u01 = perm(0u, x, 0x0c010c00u), u23 = perm(0u, x, 0x0c030c02u);
    const us2 p01 = __builtin_bit_cast(us2, u01), p23 = __builtin_bit_cast(us2, u23);
    const uint32_t q01 = __builtin_bit_cast(uint32_t, (us2)(p01 * p01)), q23 = __builtin_bit_cast(uint32_t, (us2)(p23 * p23));
    lo = perm(q23, q01, 0x06040200u);
    hi = perm(q23, q01, 0x07050301u);
}
// ... of an operand of signed bytes (pixel - 128), as signed bytes again
__device__ __forceinline__ void squares(const v4i &a, v4i &lo, v4i &hi)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t l, g;
        squares_dword((uint32_t)a[k] ^ 0x80808080u, l, g);
        lo[k] = (int)(l ^ 0x80808080u); hi[k] = (int)(g ^ 0x80808080u);
    }
}
// 0x80 (the signed byte -128) in every byte of an operand that is a null pixel (signed byte 0x80; Toeplitz padding is 0x00): a correlation
// with this plane is -128 times the correlation with the 0 / 1 null mask
__device__ __forceinline__ uint32_t null80(uint32_t x) { return x & ~((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u; }
__device__ __forceinline__ v4i null80v(const v4i &a)
{
    v4i z;
#pragma unroll
    for (int k = 0; k < 4; k++) z[k] = (int)null80((uint32_t)a[k]);
    return z;
}
// The four registers of a 16 x 16 accumulator tile (rows 4 h + 0..3 of one 16-row tile) as ONE dword of each byte plane of the next
// MFMA's B operand (signed bytes: ^ 0x80)
__device__ __forceinline__ void planes2(const v4i &R, uint32_t &p0, uint32_t &p1)
{
    const uint32_t t01 = perm((uint32_t)R[1], (uint32_t)R[0], 0x05010400u), t23 = perm((uint32_t)R[3], (uint32_t)R[2], 0x05010400u);
    p0 = perm(t23, t01, 0x05040100u) ^ 0x80808080u;
    p1 = perm(t23, t01, 0x07060302u) ^ 0x80808080u;
}
__device__ __forceinline__ void planes3(const v4i &R, uint32_t &p0, uint32_t &p1, uint32_t &p2)
{
    const uint32_t r0 = (uint32_t)R[0], r1 = (uint32_t)R[1], r2 = (uint32_t)R[2], r3 = (uint32_t)R[3];
    const uint32_t t01 = perm(r1, r0, 0x05010400u), t23 = perm(r3, r2, 0x05010400u);
    const uint32_t u01 = perm(r1, r0, 0x07030602u), u23 = perm(r3, r2, 0x07030602u);
    p0 = perm(t23, t01, 0x05040100u) ^ 0x80808080u;
    p1 = perm(t23, t01, 0x07060302u) ^ 0x80808080u;
    p2 = perm(u23, u01, 0x05040100u) ^ 0x80808080u;
}

// A band of ones as an MFMA operand: dword k of the lane, byte i <-> position x0 + xs * k + i; `fill` where lo <= position < lo + CW
__device__ __forceinline__ v4i band(int x0, int xs, int lo, int CW, uint32_t fill)
{
    v4i b;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t w = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x0 + xs * k + i;
            w |= (lo <= x && x < lo + CW) ? fill << (8 * i) : 0u;
        }
        b[k] = (int)w;
    }
    return b;
}

// sum, sum of squares and null count of the w x w chip at plane pixel (x, y), exact at every size: sub-boxes of at most 64 x 64 pixels,
// one per lane (at most nine), the three fields of each query added apart.  Wave-uniform arguments; every lane gets the result
__device__ __forceinline__ void chip_sums_u8(const SatT *__restrict__ S, int Ws, int x, int y, int w, int lane, uint32_t &sx, uint32_t &sxx, int &nulls)
{
    const int nx = (w + 63) >> 6;
    uint32_t a = 0u, b = 0u;
    int z = 0;
    if (lane < nx * nx) {
        const int j = lane / nx, i = lane - j * nx;
        const int w0 = w - 64 * i < 64 ? w - 64 * i : 64, h0 = w - 64 * j < 64 ? w - 64 * j : 64;
        const SatT q = sat_box(S, Ws, x + 64 * i, y + 64 * j, w0, h0);
        a = (uint32_t)q & ((1u << kSatSqShift8) - 1u);
        b = (uint32_t)(q >> kSatSqShift8) & ((1u << (kSatNullShift8 - kSatSqShift8)) - 1u);
        z = (int)(q >> kSatNullShift8);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); z += __shfl_xor(z, o, 64); }
    sx = (uint32_t)__builtin_amdgcn_readfirstlane((int)a); sxx = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    nulls = __builtin_amdgcn_readfirstlane(z);
}

template <class C>
__global__ __launch_bounds__(kNT, C::MINW) void match_ncc_full_chip_u8(MatchU8Args p)
{
    constexpr int KCW = C::KCW, VP = C::VP, NT = kNT, CH0 = kCH0;
    constexpr bool GEN = C::GEN;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int gidx = blockIdx.x;
    {
        const int nb = gridDim.x, per = nb >> 3;
        if (per > 0 && gidx < per * 8) gidx = (gidx & 7) * per + (gidx >> 3);   // XCD-contiguous point order
    }
    if (gidx >= p.N) return;
    if (GEN && p.point_flags[gidx] != (uint8_t)p.flag_value) return;            // flag mode: the points the clean form handed over

    const int OCW = p.ocw, R = p.full_R, S = 2 * R + 1, NC = S * S;
    const Layout L = chip_u8_layout(OCW);
    const int CW = L.CW, NPX = CW * CW, PW = L.PW, CP = L.CP, NTR = L.NTR, KCV = L.KCV, CD = L.CD;
    unsigned char *WT = smem;
    float *val = reinterpret_cast<float *>(smem);                       // [32][VP] NCC surface (over the tile, once it is consumed)
    unsigned char *CH = smem + L.off_ch;                                // the chip plane

    const unsigned char *chip_pl = p.swap ? p.p1 : p.p0;
    const unsigned char *win_pl = p.swap ? p.p0 : p.p1;
    const SatT *sat_chip = reinterpret_cast<const SatT *>(p.swap ? p.sat1 : p.sat0);
    const SatT *sat_win = reinterpret_cast<const SatT *>(p.swap ? p.sat0 : p.sat1);
    const int Wp = p.Wp, PAD = p.pad;
    // a point that leaves before its surface exists: the record (NaN or a status), every candidate slot, an all-NaN surface
    auto no_record = [&](float status) __attribute__((always_inline)) {
        if constexpr (C::ACC) { mx::stack_acc_none(p, gidx, tid, status); return; }       // (no cell; the layer counts unless refused)
        if (tid == 0) { mx::full_store(p.out + 8 * (size_t)gidx, status); mx::full_peak_store<C>(p, gidx, -1); mx::full_cand_fill<C>(p, gidx, status); }
        if constexpr (C::SURF) {
            float *sf = p.full_surf + (size_t)gidx * (size_t)NC;
            for (int k = tid; k < NC; k += NT) sf[k] = __builtin_nanf("");
        }
    };

    // ---- point header ---------------------------------------------------------------------------------------------------------------
    const double *row = p.xyuvav + (size_t)p.xy_stride * (size_t)gidx + p.xy_col;
    const int u0 = (int)row[0], v0 = (int)row[1];
    // (a point that breaks the bounds the host entry refuses -- only the _dev entry can pass one: no read, all NaN; the clean form writes it)
    if (u0 - OCW < 0 || u0 + OCW >= p.W || v0 - OCW < 0 || v0 + OCW >= p.H) { if (!GEN) no_record(__builtin_nanf("")); return; }
    const int lu = p.full_shift ? p.full_shift[2 * (size_t)gidx] : 0, lv = p.full_shift ? p.full_shift[2 * (size_t)gidx + 1] : 0;
    const int D2 = CW + 2 * R;                                          // the search box is D2 x D2 pixels; the tile's cell s_t = s + R
    const int cu0 = u0 - OCW + PAD, cv0 = v0 - OCW + PAD;               // plane position of chip pixel (0, 0)
    const int wu0 = u0 + p.off_u + lu - R - OCW + PAD, wv0 = v0 + p.off_v + lv - R - OCW + PAD;      // ... of box (and tile) pixel (0, 0)
    if (wu0 < 0 || wv0 < 0 || wu0 + D2 > p.W + 2 * PAD || wv0 + D2 > p.H + 2 * PAD) { if (!GEN) no_record(__builtin_nanf("")); return; }

    uint32_t SX, SXX;
    int chip_nulls;
    chip_sums_u8(sat_chip, p.sat_ws, cu0, cv0, CW, lane, SX, SXX, chip_nulls);
    const int win_nulls = __builtin_amdgcn_readfirstlane(sat_nulls_u8(sat_win, p.sat_ws, wu0, wv0, D2, D2, lane));
    if constexpr (!GEN) {
        if (chip_nulls != 0 || win_nulls != 0) {                        // the masked form's point
            if (tid == 0) p.mx_flags[gidx] = kMxNulls;
            return;
        }
    } else {
        // validity (a6, :605-644): nulls of the chip / of the whole search box
        const float max_ratio = 0.8f;
        const float rc = (float)chip_nulls / (float)NPX;
        const float rw = (float)win_nulls / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }
    [[maybe_unused]] const bool wn = GEN && win_nulls != 0, cn = GEN && chip_nulls != 0;

    // ---- stage the tile: window pixels (x, y), x < SW, y < KW, as signed bytes b - 128 (both waves); the chip plane: zeros -----------
    {
        const int NSEG = L.SW / 16, TTASK = L.KW * NSEG;                // (tile rows >= KW and columns >= SW are only ever weighted 0: left as they are)
        const float inv_nseg = 1.0f / (float)NSEG;                      // t / NSEG for t < 2,304, NSEG <= 12: (t + 1/2) / NSEG lies 1 / 24 from an integer
        const int tsh = wu0 & 3;
        const uint32_t *tgb = reinterpret_cast<const uint32_t *>(win_pl + (size_t)wv0 * Wp + (wu0 - tsh));
        // (the tile reaches up to 31 - 2R rows and 50 - 2R columns past the search box, which may end at the plane's last row: the loads
        //  are clamped to the plane; what a clamped load brings only reaches cells outside the search range)
        const uint32_t tlim = (uint32_t)(((size_t)(p.H + 2 * PAD) * (size_t)Wp - ((size_t)wv0 * Wp + (size_t)(wu0 - tsh))) / 4 - 1);
#pragma unroll 1
        for (int t0 = tid; t0 < TTASK; t0 += 4 * NT) {
            uint32_t td[4][5];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = t0 + NT * k;
                const bool on = t < TTASK;
                const int y = (int)(((float)t + 0.5f) * inv_nseg), q = t - NSEG * y;
                const uint32_t go = on ? (uint32_t)y * (uint32_t)(Wp >> 2) + 4u * (uint32_t)q : 0u;
#pragma unroll
                for (int j = 0; j < 5; j++) td[k][j] = tgb[min(go + (uint32_t)j, tlim)];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = t0 + NT * k;
                const int y = (int)(((float)t + 0.5f) * inv_nseg), q = t - NSEG * y;
                if (t < TTASK) {
                    uint4 w;
                    w.x = alignb(td[k][1], td[k][0], tsh) ^ 0x80808080u;
                    w.y = alignb(td[k][2], td[k][1], tsh) ^ 0x80808080u;
                    w.z = alignb(td[k][3], td[k][2], tsh) ^ 0x80808080u;
                    w.w = alignb(td[k][4], td[k][3], tsh) ^ 0x80808080u;
                    *reinterpret_cast<uint4 *>(WT + y * PW + 16 * q) = w;
                }
            }
        }
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < L.CHB / 16; i += NT) reinterpret_cast<uint4 *>(CH)[i] = z4;
    }
    __syncthreads();
    // ---- the chip plane: CW rows of (a ^ 0x80), aligned dwords of the chip's rows ---------------------------------------------------
    {
        const int CTASK = CW * CD;
        const float inv_cd = 1.0f / (float)CD;                          // t / CD for t < 6,601, CD <= 41: (t + 1/2) / CD lies 1 / 82 from an integer
        const int csh = cu0 & 3;
        const uint32_t *cgb = reinterpret_cast<const uint32_t *>(chip_pl + (size_t)cv0 * Wp + (cu0 - csh));
        const uint32_t lastm = L.LASTN >= 4 ? 0xffffffffu : ((1u << (8 * L.LASTN)) - 1u);
#pragma unroll 1
        for (int t0 = tid; t0 < CTASK; t0 += 4 * NT) {
            uint32_t clo[4], chi[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = t0 + NT * k;
                const bool on = t < CTASK;
                const int r = (int)(((float)t + 0.5f) * inv_cd), j = t - CD * r;
                const uint32_t go = on ? (uint32_t)r * (uint32_t)(Wp >> 2) + (uint32_t)j : 0u;
                clo[k] = cgb[go]; chi[k] = cgb[go + 1u];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = t0 + NT * k;
                const int r = (int)(((float)t + 0.5f) * inv_cd), j = t - CD * r;
                if (t < CTASK) {
                    const uint32_t a = alignb(chi[k], clo[k], csh);
                    const uint32_t m = (j == CD - 1) ? lastm : 0xffffffffu;
                    *reinterpret_cast<uint32_t *>(CH + CH0 + CP * r + 4 * j) = (a ^ 0x80808080u) & m;
                }
            }
        }
    }
    __syncthreads();

    // lane (n, h) of wave w: cell column s = 16 w + n; byte i of K chunk c <-> window column 16 w + 64 c + 16 h + i
    const int n = lane & 15, h = lane >> 4;
    const unsigned char *arow = WT + n * PW + 16 * wave + 16 * h;       // A operand: tile row r + 16 mt + n
    const int boff = CH0 + 16 * h - n;                                   // B operand: chip-row bytes 64 c + 16 h - n + i
    const uint32_t bsh = (uint32_t)boff & 3u;
    const unsigned char *brow = CH + (boff & ~3);
    // the band of ones of the row-box sums (B operand: 1 where the byte is a window column of the cell's box, i.e. where the Toeplitz row
    // holds a chip pixel; the wave index cancels)
    v4i hb[KCW];
#pragma unroll
    for (int c = 0; c < KCW; c++) hb[c] = band(64 * c + 16 * h, 4, n, CW, 1u);

    // ---- the product surface (and the null correlations): the double-buffered row loop of match_ncc_dlc_mx ---------------------------
    const v4i zero4 = {0, 0, 0, 0};
    // accumulators (two 16 x 16 tiles each): sum a'b'; masked form, window nulls zb: sum zb a', sum zb (a^2 & 255)', sum zb (a^2 >> 8)';
    // chip nulls za: sum b' za, sum (b^2 & 255)' za, sum (b^2 >> 8)' za, and sum zb za
    v4i acc[2] = {zero4, zero4}, accz[2] = {zero4, zero4}, accl[2] = {zero4, zero4}, acch[2] = {zero4, zero4};
    v4i accy[2] = {zero4, zero4}, accyl[2] = {zero4, zero4}, accyh[2] = {zero4, zero4}, acczz[2] = {zero4, zero4};
    (void)accz; (void)accl; (void)acch; (void)accy; (void)accyl; (void)accyh; (void)acczz;
    {
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
        // (the null-plane operands are 0x80 = -128 per null: their correlations come out times -128, their product times 16384)
        auto consume = [&](const RowOps &o, bool chip_row) __attribute__((always_inline)) {
            v4i b[KCW];
#pragma unroll
            for (int c = 0; c < KCW; c++)
#pragma unroll
                for (int k = 0; k < 4; k++) b[c][k] = (int)alignb(o.d[c][k + 1], o.d[c][k], bsh);
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int c = 0; c < KCW; c++) acc[m] = mfma(o.a[m][c], b[c], acc[m]);
            if constexpr (GEN) {
#pragma unroll
                for (int c = 0; c < KCW; c++) {
                    v4i z[2];
                    z[0] = null80v(o.a[0][c]); z[1] = null80v(o.a[1][c]);
                    if (wn && chip_row) {
                        // the byte planes of a^2 from the Toeplitz row itself; its padding (0x00, which would square as the pixel 128) masked out
                        // (the zero row behind the chip is all such bytes, under the band as well: it takes no part)
                        v4i al, ah;
                        squares(b[c], al, ah);
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t bm = (uint32_t)hb[c][k] * 255u;
                            al[k] = (int)((uint32_t)al[k] & bm); ah[k] = (int)((uint32_t)ah[k] & bm);
                        }
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            accz[m] = mfma(z[m], b[c], accz[m]); accl[m] = mfma(z[m], al, accl[m]); acch[m] = mfma(z[m], ah, acch[m]);
                        }
                    }
                    if (cn) {
                        const v4i za = null80v(b[c]);              // (a padding byte is 0x00, a null chip pixel 0x80)
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            v4i lo, hi;
                            squares(o.a[m][c], lo, hi);
                            accy[m] = mfma(o.a[m][c], za, accy[m]); accyl[m] = mfma(lo, za, accyl[m]); accyh[m] = mfma(hi, za, accyh[m]);
                            acczz[m] = mfma(z[m], za, acczz[m]);
                        }
                    }
                }
            }
        };
        RowOps o0, o1;
        issue(0, o0);
#pragma unroll 1
        for (int r = 0; r < L.CWE; r += 2) {
            issue(r + 1, o1);
            __builtin_amdgcn_sched_barrier(0);
            consume(o0, true);
            __builtin_amdgcn_sched_barrier(0);
            issue(r + 2 < L.CWE ? r + 2 : r + 1, o0);           // (the last trip re-reads a row: nothing consumes it)
            __builtin_amdgcn_sched_barrier(0);
            consume(o1, r + 1 < CW);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (GEN) {        // the two byte planes of each squared operand back into one sum (and out of the -128 scale)
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                accl[m][i] = ((-accl[m][i]) >> 7) + 256 * ((-acch[m][i]) >> 7);
                accyl[m][i] = ((-accyl[m][i]) >> 7) + 256 * ((-accyh[m][i]) >> 7);
            }
    }

    // ---- window-side box sums of the wave's 32 x 16 cells: sum b, sum b^2 (and the null count) ------------------------------------
    //      row-box sums R[y][s] = sum_{x = s}^{s + CW - 1} q[y][x] by MFMA (A = 16 tile rows, B = the band of ones), then
    //      Box[dy][s] = sum_{y = dy}^{dy + CW - 1} R[y][s] by MFMA (A = the band of ones, B = the byte planes of R).  NTR <= 12 row tiles,
    //      KCV <= 3 chunks: unrolled to the largest of the KCW class, the tiles and chunks beyond the run-time counts skipped (wave-uniform)
    v4i boxb[2], boxq[2], boxz[2] = {zero4, zero4};
    {
        constexpr int MT = max_ntr(KCW), MC = (MT + 3) / 4;
        auto tile_a = [&](int t, v4i (&a)[KCW]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < KCW; c++) a[c] = *reinterpret_cast<const v4i *>(arow + 16 * t * PW + 64 * c);
        };
        // A operand of the vertical sums -- cell row dy = 16 m + n; K slot (h, i) of chunk c <-> tile row y = 64 c + 16 (i >> 2) + 4 h + (i & 3)
        auto vband = [&](int m, int c) __attribute__((always_inline)) -> v4i { return band(64 * c + 4 * h, 16, 16 * m + n, CW, 1u); };
        {   // sum b (and the null count)
            v4i p0[MC], p1[MC], pz[MC];
#pragma unroll
            for (int t = 0; t < 4 * MC; t++) {
                uint32_t q0 = 0, q1 = 0, qz = 0;
                if (t < MT && t < NTR) {
                    v4i a[KCW];
                    tile_a(t, a);
                    v4i Rs = zero4;
#pragma unroll
                    for (int c = 0; c < KCW; c++) Rs = mfma(a[c], hb[c], Rs);
#pragma unroll
                    for (int i = 0; i < 4; i++) Rs[i] += 128 * CW;
                    planes2(Rs, q0, q1);
                    if (GEN && wn) {                          // the row counts of the nulls (the null plane is -128 per null), <= 161: one plane in offset form
                        v4i Z = zero4;
#pragma unroll
                        for (int c = 0; c < KCW; c++) Z = mfma(null80v(a[c]), hb[c], Z);
#pragma unroll
                        for (int i = 0; i < 4; i++) Z[i] = (-Z[i]) >> 7;
                        uint32_t unused;
                        planes2(Z, qz, unused);
                    }
                }
                p0[t >> 2][t & 3] = (int)q0; p1[t >> 2][t & 3] = (int)q1; pz[t >> 2][t & 3] = (int)qz;
            }
#pragma unroll
            for (int m = 0; m < 2; m++) {
                v4i v0 = zero4, v1 = zero4, vz = zero4;
#pragma unroll
                for (int c = 0; c < MC; c++) {
                    if (c < KCV) {
                        const v4i vb = vband(m, c);
                        v0 = mfma(vb, p0[c], v0); v1 = mfma(vb, p1[c], v1);
                        if (GEN && wn) vz = mfma(vb, pz[c], vz);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    boxb[m][i] = (v0[i] + 128 * CW) + 256 * (v1[i] + 128 * CW);
                    if (GEN && wn) boxz[m][i] = vz[i] + 128 * CW;
                }
            }
        }
        {   // sum b^2
            v4i p0[MC], p1[MC], p2[MC];
#pragma unroll
            for (int t = 0; t < 4 * MC; t++) {
                uint32_t q0 = 0, q1 = 0, q2 = 0;
                if (t < MT && t < NTR) {
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
                for (int c = 0; c < MC; c++) {
                    if (c < KCV) {
                        const v4i vb = vband(m, c);
                        v0 = mfma(vb, p0[c], v0); v1 = mfma(vb, p1[c], v1); v2 = mfma(vb, p2[c], v2);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) boxq[m][i] = (v0[i] + 128 * CW) + 256 * (v1[i] + 128 * CW) + 65536 * (v2[i] + 128 * CW);
            }
        }
    }
    __syncthreads();                                        // the tile's bytes become the NCC surface

    // ---- NCC of the 8 cells of this lane (:734): exact integer sums, the f64 formula rounded to f32 (match_full_tail.h) --------------
    {
        const int sx_col = 16 * wave + n;
        const int Na = chip_nulls;
        const double dn0 = (double)(NPX - Na), dsx0 = (double)SX, va0 = dn0 * (double)SXX - dsx0 * dsx0;
        auto cell_in = [&](int m, int i, double &dn, double &dsx, double &va, double &sxy, int &sy, int &syy) __attribute__((always_inline)) {
            sy = boxb[m][i]; syy = boxq[m][i];
            // sum ab over all chip positions (a null is a zero factor), in f64: the partial sum comes within 1.5 % of 2^31
            sxy = ((double)acc[m][i] + 128.0 * ((double)SX + (double)sy)) - 16384.0 * (double)NPX;
            dn = dn0; dsx = dsx0; va = va0;
            if (GEN && cn) {                                   // chip nulls take window pixels out of sy, syy
                sy -= ((-accy[m][i]) >> 7) + 128 * Na;
                syy -= accyl[m][i] + (128 + 256 * 128) * Na;
            }
            if (GEN && wn) {                                   // window nulls take chip pixels out of n, sx, sxx
                const int nz = boxz[m][i];
                const int ca = ((-accz[m][i]) >> 7) + 128 * nz, caa = accl[m][i] + (128 + 256 * 128) * nz;
                dn = (double)(NPX - Na - nz + (cn ? (acczz[m][i] >> 14) : 0)); dsx = (double)((int)SX - ca);
                va = dn * (double)((int)SXX - caa) - dsx * dsx;
            }
        };
        uint32_t amb = 0u;
#pragma unroll
        for (int ci = 0; ci < 8; ci++) {
            const int m = ci >> 2, i = ci & 3, ry = 16 * m + 4 * h + i;
            double dn, dsx, va, sxy; int sy, syy;
            cell_in(m, i, dn, dsx, va, sxy, sy, syy);
            const double dsy = (double)sy;
            const double num = dn * sxy - dsx * dsy;
            const double P = va * (dn * (double)syy - dsy * dsy);
            bool redo;
            const double q = mx::ncc_quot_fast(num, P, redo);
            if (redo) amb |= 1u << ci;
            val[ry * VP + sx_col] = (float)q;
            if constexpr (GEN) __builtin_amdgcn_sched_barrier(0);      // (masked form: one cell at a time)
        }
        if (__any(amb != 0u)) {                            // rare (2^-15 of the cells): the reference's own operations
#pragma unroll
            for (int ci = 0; ci < 8; ci++) {
                if (!__any((amb >> ci) & 1u)) continue;
                const int m = ci >> 2, i = ci & 3, ry = 16 * m + 4 * h + i;
                double dn, dsx, va, sxy; int sy, syy;
                cell_in(m, i, dn, dsx, va, sxy, sy, syy);
                const double dsy = (double)sy;
                const double num = dn * sxy - dsx * dsy;
                const double den = mx::ncc_den_exact(va * (dn * (double)syy - dsy * dsy));
                if ((amb >> ci) & 1u) val[ry * VP + sx_col] = mx::ncc_quot_exact(num, den);
            }
        }
    }
    __syncthreads();
    if constexpr (C::ACC) {                                 // the surface into the stack, in the SURF store's place; no tail
        mx::stack_acc_any<NT, VP>(p, val, gidx, S, tid);     // (resampled where the layer is a scaled one: a launch-uniform branch)
        return;
    }
    if constexpr (C::SURF) {                                // the surface in k order (u outer): coalesced stores, LDS reads at stride VP
        float *sf = p.full_surf + (size_t)gidx * (size_t)NC;
        for (int k = tid; k < NC; k += NT) {
            const int x = k / S, y = k - S * x;
            sf[k] = val[y * VP + x];
        }
    }
    if (wave != 0) return;
    mx::full_tail<C>(p, val, gidx, lu, lv, lane);
    if constexpr (C::MULTI) mx::full_tail_multi<C>(p, val, gidx, lu, lv, lane);
}

template <class C>
static hipError_t launch_one(const MatchU8Args &a, hipStream_t stream)
{
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    const int lds = chip_u8_layout(a.ocw).lds;
    if (lds > 60 * 1024) {              // near or beyond the default limit of LDS (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_full_chip_u8<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_full_chip_u8<C>, dim3(nb), dim3(kNT), lds, stream, a);
    return hipGetLastError();
}

template <bool GEN, bool MULTI, bool SURF>
static hipError_t launch_kcw(const MatchU8Args &a, hipStream_t stream)
{
    switch (chip_u8_layout(a.ocw).KCW) {
    case 1: return launch_one<Cfg<1, GEN, MULTI, SURF>>(a, stream);
    case 2: return launch_one<Cfg<2, GEN, MULTI, SURF>>(a, stream);
    case 3: return launch_one<Cfg<3, GEN, MULTI, SURF>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

template <bool GEN>
static hipError_t launch_kcw_acc(const MatchU8Args &a, hipStream_t stream)
{
    switch (chip_u8_layout(a.ocw).KCW) {
    case 1: return launch_one<AccCfg<1, GEN>>(a, stream);
    case 2: return launch_one<AccCfg<2, GEN>>(a, stream);
    case 3: return launch_one<AccCfg<3, GEN>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

template <bool GEN>
static hipError_t launch_kcw_peak(const MatchU8Args &a, hipStream_t stream)
{
    switch (chip_u8_layout(a.ocw).KCW) {
    case 1: return launch_one<PeakCfg<1, GEN>>(a, stream);
    case 2: return launch_one<PeakCfg<2, GEN>>(a, stream);
    case 3: return launch_one<PeakCfg<3, GEN>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

// the PEAK forms: the same two launches
static hipError_t launch_forms_peak(MatchU8Args a, int forms, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    if (forms & 1) e = launch_kcw_peak<false>(a, stream);
    a.point_flags = a.mx_flags; a.flag_value = kMxNulls;
    if (e == hipSuccess && (forms & 2)) e = launch_kcw_peak<true>(a, stream);
    return e;
}

// the accumulating forms: the same two launches, the clean form's hand-over of flagged points unchanged
static hipError_t launch_forms_acc(MatchU8Args a, int forms, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    if (forms & 1) e = launch_kcw_acc<false>(a, stream);
    a.point_flags = a.mx_flags; a.flag_value = kMxNulls;
    if (e == hipSuccess && (forms & 2)) e = launch_kcw_acc<true>(a, stream);
    return e;
}

// the clean form over all points, then the masked form in flag mode over the points it flagged
template <bool MULTI, bool SURF>
static hipError_t launch_forms(MatchU8Args a, int forms, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    if (forms & 1) e = launch_kcw<false, MULTI, SURF>(a, stream);
    a.point_flags = a.mx_flags; a.flag_value = kMxNulls;
    if (e == hipSuccess && (forms & 2)) e = launch_kcw<true, MULTI, SURF>(a, stream);
    return e;
}

}  // namespace fchip8

bool full_chip_u8_layout(int ocw, int out[4])
{
    if (ocw < 1 || ocw > kFullChipMaxOcw) return false;
    const fchip8::Layout l = fchip8::chip_u8_layout(ocw);
    out[0] = l.KCW; out[1] = l.NTR; out[2] = l.KCV; out[3] = l.lds;
    return true;
}

hipError_t launch_match_full_chip_u8(MatchU8Args a, int forms, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || !a.mx_flags || !a.sat0 || !a.sat1 || a.full_R < 1 || a.full_R > 15 || a.ocw < 1 || a.ocw > kFullChipMaxOcw)
        return hipErrorInvalidValue;
    a.point_flags = nullptr;
    if (forms & kFormsAcc) {            // the stack's planes in the list-mode slots; nothing else is written
        if (!a.stk_sum || !a.stk_cnt || !a.stk_lay || a.out || a.full_cand || a.full_surf || a.full_peak) return hipErrorInvalidValue;
        if (a.stk_shift && !mx::stack_acc_scaled_ok(a)) return hipErrorInvalidValue;
        return fchip8::launch_forms_acc(a, forms, stream);
    }
    if (a.full_peak) {                  // the arg-max cells: with the record alone
        if (a.full_cand || a.full_surf) return hipErrorInvalidValue;
        return fchip8::launch_forms_peak(a, forms, stream);
    }
    if (a.full_cand) {
        if (a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks) return hipErrorInvalidValue;
        return a.full_surf ? fchip8::launch_forms<true, true>(a, forms, stream) : fchip8::launch_forms<true, false>(a, forms, stream);
    }
    return a.full_surf ? fchip8::launch_forms<false, true>(a, forms, stream) : fchip8::launch_forms<false, false>(a, forms, stream);
}

}  // namespace mimc3
