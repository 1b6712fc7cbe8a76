// match_full_chip_u16_kernel.hip -- exhaustive-search NCC offsets for gfx950 on SCALED-INTEGER pairs (u16 planes, q = value * 2^s < 4096:
// 12-bit DN, and the d/dx, d/dy and Laplacian forms of an 8-bit pair) at ANY chip half-width 1 <= ocw <= 80, on the matrix cores
// (mimc3_match_ncc_full_chip_planes).  ocw is a RUN-TIME value here.
//
// It is match_full_chip_u8_kernel.hip (which has the scheme: the Toeplitz-band GEMM on v_mfma_i32_16x16x64_i8 over the 32 x 32 cell tile
// with origin c - R, two waves per point, the window-side box sums on the same pipe against two bands of ones formed from the lane index,
// the finish and tails of match_full_tail.h as they stand, the surface in LDS at pitch 33) with every pixel as TWO 6-bit planes:
//   q = 64 h + l,  h, l <= 63  -- both planes are non-negative i8 values, so no ^ 0x80 offset and no offset terms on the pixel planes;
//   sum ab = 4096 HH + 64 (HL + LH) + LL,  HL + LH = SS - HH - LL  with  SS = sum (h + l)(h' + l')  (h + l <= 126 is still an i8):
//   three correlations per K chunk, the sum planes formed in registers, the result put together in 64-bit integers.
//   staging    the u16 pixels are split at staging: two tiles and two chip planes of bytes, each in the u8 kernel's layout -- the layout
//              of that kernel with both parts doubled (chip_u16_layout(ocw), the one expression kernel, launch and static checks share).
//   template   KCW, the K chunks (64 window columns) per chip row: 1 (ocw <= 24), 2 (ocw <= 56) or 3.
//   box sums   a row-box sum of q (< 2^20) goes on as three byte planes, one of q^2 (above 2^31, below 2^32: kept in a u32) as four, a row's
//              null count (<= 161) as one; these byte planes are in offset form (^ 0x80, + 128 CW per plane afterwards) as in the u8
//              kernel.  q^2 of four pixels is formed in registers from the two plane dwords and split into its three byte planes.
//   tables     the packed u16 table (sat_kernel.h: q | q^2 << 25) is exact for one query only while sum q < 2^25 -- 8,194 saturated pixels,
//              CW <= 89 -- so the chip's sums are ALWAYS taken in sub-boxes of at most 64 x 64 pixels, one per lane, the two fields added
//              apart in 64 bits (chip_sums_u16).  The null counts come from the u32 null table, exact for any box.
// Two forms, as there: the clean form runs over all points and flags a point that holds a null in its chip or its search box (kMxNulls in
// mx_flags); the masked form runs behind it in flag mode.  A null is q == 0, both planes 0: sum ab needs no mask; the other five sums are
// the clean ones minus correlations with zb = [b == 0] (window) and za = [a == 0] (chip) --
//   sum zb, sum zb a (two planes), sum zb a^2 (three byte planes)   take chip pixels out of n, sx, sxx under window nulls,
//   sum b za (two planes), sum b^2 za (three byte planes), sum zb za  take window pixels out of sy, syy (and put back what n lost twice)
// -- every extra operand formed in registers.  A chip plane's padding is 0 like a null: za is masked by the band of chip bytes, and the
// zero row behind the odd chip takes no part in the za and a^2 groups.  The groups are skipped wave-uniformly.
// The finish is written as match_full_chip_kernel.hip writes it (num = dn sxy - dsx dsy, va, vb, P = va vb in f64 on the exact integer
// sums; -ffp-contract=off): from CW = 153 on n sum ab and (sum a)^2 can pass 2^53 on near-saturated data and the products ROUND -- the
// bytes are the float kernel's because both do the same operations on the same exact inputs (a power-of-two pixel scale commutes with
// every rounding).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "sat_kernel.h"
#include "match_full_tail.h"
#include "stack_acc.h"

namespace mimc3 {

namespace fchip16 {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned long long SatT;

constexpr int kNT = 128;                            // two wave64 per grid point
constexpr int kVP = 33;                             // pitch (words) of the NCC surface
constexpr int kValBytes = 4 * 32 * kVP;
constexpr int kCH0 = 16;                            // leading zeros of a chip plane (row 0's left padding)

static_assert(kFullChipMaxOcw == 80, "the bounds below are those of CW = 161");
static_assert(161ll * 161 * 63 * 63 == 102880449ll && 161ll * 161 * 63 * 63 < (1ll << 27), "a plane correlation");
static_assert(161ll * 161 * 126 * 126 == 411521796ll && 161ll * 161 * 126 * 126 < (1ll << 29), "the (h + l)(h' + l') correlation");
static_assert(161ll * 161 * 4095 * 4095 == 434669897025ll && 161ll * 161 * 4095 * 4095 < (1ll << 39) && 161ll * 161 * 4095 * 4095 > (1ll << 31),
              "the true sum ab (and a box sum of q^2): 64 bits");
static_assert(161ll * 4095 == 659295ll && 161ll * 4095 < (1ll << 20), "a row-box sum of q: three byte planes");
static_assert(161ll * 4095 * 4095 == 2699813025ll && 161ll * 4095 * 4095 > (1ll << 31) && 161ll * 4095 * 4095 < (1ll << 32),
              "a row-box sum of q^2: a u32, four byte planes");
static_assert(161ll * 161 * 4095 < (1ll << 27), "a box sum of q: an i32");
static_assert(161ll * 161 * 255 < (1ll << 23), "a correlation of a byte plane (offset form: |x - 128| <= 128) with a null indicator");
static_assert(64ll * 64 * 4095 < (1ll << kSatSqShift16) && 64ll * 64 * 4095 * 4095 < (1ll << (64 - kSatSqShift16)),
              "a 64 x 64 sub-box fits both fields of the packed table");
static_assert(89ll * 89 * 4095 < (1ll << kSatSqShift16) && 91ll * 91 * 4095 > (1ll << kSatSqShift16), "one query is exact up to ocw 44 only");

struct Layout {
    int CW, KW, KCW, SW, PW, NTR, KCV, CD, LASTN, CP, CWE, CHB, TB, off_tl, off_ch, off_cl, lds;
};

// the one expression of the layout: the u8 kernel's, with a second tile and a second chip plane
__host__ __device__ constexpr Layout chip_u16_layout(int ocw)
{
    Layout l{};
    l.CW = 2 * ocw + 1;
    l.KW = l.CW + 31;                               // window columns (and rows) the 32 x 32 cells of a tile reach
    l.KCW = (l.CW + 15 + 63) / 64;                  // K chunks per chip row and 16 x 16 cell tile
    const int RDW = 16 + 64 * l.KCW;                // bytes of a tile row some wave reads
    l.SW = (l.KW + 15) & ~15;                       // bytes of a tile row that are staged
    const int PW0 = RDW > l.SW ? RDW : l.SW;
    l.PW = ((PW0 / 16) & 1) ? PW0 : PW0 + 16;       // pitch 16 x odd
    l.NTR = (l.KW + 15) / 16;                       // 16-row tiles of the row-box sums
    l.KCV = (l.NTR + 3) / 4;                        // K chunks (64 tile rows) of the vertical sums
    l.CD = (l.CW + 3) / 4;                          // dwords per chip-plane row
    l.LASTN = l.CW - 4 * (l.CD - 1);                // valid bytes of a chip row's last dword
    const int CP0 = (l.CW + 15 + 3) & ~3;
    l.CP = CP0 > 64 * l.KCW ? CP0 : 64 * l.KCW;     // chip plane pitch: a row's right padding is the next row's left padding
    l.CWE = l.CW + 1;                               // chip rows the product loop walks, two per trip: the all-zero row behind the odd chip
    l.CHB = (kCH0 + l.CWE * l.CP + 16 + 15) & ~15;  // one chip plane (+ the read-ahead of the last row's last lane)
    const int ldsw = (16 * l.NTR + 1) * l.PW;       // one tile (+ the row the product loop's zero chip row reads)
    l.TB = ((ldsw > kValBytes ? ldsw : kValBytes) + 15) & ~15;          // the surface reuses the first tile's bytes
    l.off_tl = l.TB;                                // the tile of l (the tile of h at 0)
    l.off_ch = 2 * l.TB;                            // the chip plane of h
    l.off_cl = l.off_ch + l.CHB;                    // ... of l
    l.lds = l.off_cl + l.CHB;
    return l;
}

// the most 16-row tiles of the box sums in a KCW class: what the box-sum loops are unrolled to
__host__ __device__ constexpr int max_ntr(int kcw) { return kcw >= 3 ? 12 : (64 * kcw + 16 + 15) / 16; }

constexpr bool layouts_fit()
{
    for (int ocw = 1; ocw <= kFullChipMaxOcw; ocw++) {
        const Layout l = chip_u16_layout(ocw);
        if (l.KCW < 1 || l.KCW > 3 || l.NTR > 12 || l.KCV > 3 || l.lds > 160 * 1024) return false;
        if (l.KW > 16 * l.NTR || l.SW > l.PW || 16 + 64 * l.KCW > l.PW || l.CP < l.CW + 15 || l.CP < 64 * l.KCW) return false;
        if (l.LASTN < 1 || l.LASTN > 4 || 4 * l.CD > l.CP) return false;
        if ((l.KCW == 1) != (ocw <= 24) || (l.KCW == 3) != (ocw >= 57)) return false;
        if (l.NTR > max_ntr(l.KCW)) return false;
        if ((16 * l.NTR + 1) * l.PW > l.TB || kValBytes > l.TB) return false;
    }
    return true;
}
static_assert(layouts_fit(), "every ocw fits its LDS, and the reads stay inside the rows and planes of the layout");
static_assert(2 * chip_u16_layout(56).lds <= 160 * 1024, "two workgroups per CU up to the largest chip of the two-chunk class");

template <int KCW_, bool GEN_, bool MULTI_, bool SURF_>
struct Cfg {                                        // (VP, PEAK, MULTI: what match_full_tail.h asks of a configuration)
    static constexpr int KCW = KCW_, VP = kVP;
    static constexpr bool GEN = GEN_, PEAK = false, MULTI = MULTI_, SURF = SURF_;
    // occupancy target, waves per SIMD: the most that leaves the kernel without scratch (the masked form of two chunks spills at 2)
    static constexpr int MINW = GEN_ ? (KCW_ == 1 ? 2 : 1) : (KCW_ == 1 ? 3 : KCW_ == 2 ? 2 : 1);
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

// the four registers of a 16 x 16 accumulator tile as one dword of each byte plane of the next MFMA's B operand (signed bytes: ^ 0x80)
__device__ __forceinline__ void planes4(const v4i &R, uint32_t &p0, uint32_t &p1, uint32_t &p2, uint32_t &p3)
{
    const uint32_t r0 = (uint32_t)R[0], r1 = (uint32_t)R[1], r2 = (uint32_t)R[2], r3 = (uint32_t)R[3];
    const uint32_t t01 = perm(r1, r0, 0x05010400u), t23 = perm(r3, r2, 0x05010400u);
    const uint32_t u01 = perm(r1, r0, 0x07030602u), u23 = perm(r3, r2, 0x07030602u);
    p0 = perm(t23, t01, 0x05040100u) ^ 0x80808080u;
    p1 = perm(t23, t01, 0x07060302u) ^ 0x80808080u;
    p2 = perm(u23, u01, 0x05040100u) ^ 0x80808080u;
    p3 = perm(u23, u01, 0x07060302u) ^ 0x80808080u;
}
// q^2 of the four pixels of a plane-dword pair (q = 64 h + l) as its three byte planes, signed bytes (^ 0x80)
__device__ __forceinline__ void squares_dword(uint32_t h, uint32_t l, uint32_t &p0, uint32_t &p1, uint32_t &p2)
{
    const uint32_t q01 = (perm(0u, h, 0x0c010c00u) << 6) + perm(0u, l, 0x0c010c00u);
    const uint32_t q23 = (perm(0u, h, 0x0c030c02u) << 6) + perm(0u, l, 0x0c030c02u);
    v4i s;
    s[0] = (int)__umul24(q01 & 0xffffu, q01 & 0xffffu); s[1] = (int)__umul24(q01 >> 16, q01 >> 16);
    s[2] = (int)__umul24(q23 & 0xffffu, q23 & 0xffffu); s[3] = (int)__umul24(q23 >> 16, q23 >> 16);
    uint32_t unused;
    planes4(s, p0, p1, p2, unused);
}
__device__ __forceinline__ void squares(const v4i &h, const v4i &l, v4i &p0, v4i &p1, v4i &p2)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t a, b, c;
        squares_dword((uint32_t)h[k], (uint32_t)l[k], a, b, c);
        p0[k] = (int)a; p1[k] = (int)b; p2[k] = (int)c;
    }
}
// 1 in every byte of x that is 0 (no carry between the bytes, whatever they hold)
__device__ __forceinline__ uint32_t null01(uint32_t x) { return (~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u; }
__device__ __forceinline__ v4i null01v(const v4i &h, const v4i &l)
{
    v4i z;
#pragma unroll
    for (int k = 0; k < 4; k++) z[k] = (int)null01((uint32_t)h[k] | (uint32_t)l[k]);
    return z;
}
__device__ __forceinline__ v4i addv(const v4i &h, const v4i &l) { return h + l; }       // (bytes <= 63 + 63: no carry)

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

// sum and sum of squares of the w x w chip at plane pixel (x, y), exact at every size: sub-boxes of at most 64 x 64 pixels, one per lane
// (at most nine), the two fields of each query added apart.  Wave-uniform arguments; every lane gets the result
__device__ __forceinline__ void chip_sums_u16(const SatT *__restrict__ S, int Ws, int x, int y, int w, int lane, uint32_t &sx, unsigned long long &sxx)
{
    const int nx = (w + 63) >> 6;
    uint32_t a = 0u;
    unsigned long long b = 0ull;
    if (lane < nx * nx) {
        const int j = lane / nx, i = lane - j * nx;
        const int w0 = w - 64 * i < 64 ? w - 64 * i : 64, h0 = w - 64 * j < 64 ? w - 64 * j : 64;
        const SatT q = sat_box(S, Ws, x + 64 * i, y + 64 * j, w0, h0);
        a = (uint32_t)q & ((1u << kSatSqShift16) - 1u);
        b = q >> kSatSqShift16;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        const uint32_t blo = __shfl_xor((uint32_t)b, o, 64), bhi = __shfl_xor((uint32_t)(b >> 32), o, 64);
        b += ((unsigned long long)bhi << 32) | blo;
    }
    sx = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
    sxx = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
}

// the four pixels of two u16-pair dwords as one dword of each plane
__device__ __forceinline__ void split4(uint32_t d0, uint32_t d1, uint32_t &h, uint32_t &l)
{
    h = perm((d1 >> 6) & 0x003f003fu, (d0 >> 6) & 0x003f003fu, 0x06040200u);
    l = perm(d1 & 0x003f003fu, d0 & 0x003f003fu, 0x06040200u);
}

template <class C>
__global__ __launch_bounds__(kNT, C::MINW) void match_ncc_full_chip_u16(MatchU8Args p)
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
    const Layout L = chip_u16_layout(OCW);
    const int CW = L.CW, NPX = CW * CW, PW = L.PW, CP = L.CP, NTR = L.NTR, KCV = L.KCV, CD = L.CD;
    unsigned char *WTH = smem, *WTL = smem + L.off_tl;                  // the tiles of h and l
    float *val = reinterpret_cast<float *>(smem);                       // [32][VP] NCC surface (over the first tile, once both are consumed)
    unsigned char *CHH = smem + L.off_ch, *CHL = smem + L.off_cl;       // the chip planes

    const unsigned short *chip_pl = reinterpret_cast<const unsigned short *>(p.swap ? p.p1 : p.p0);
    const unsigned short *win_pl = reinterpret_cast<const unsigned short *>(p.swap ? p.p0 : p.p1);
    const SatT *sat_chip = reinterpret_cast<const SatT *>(p.swap ? p.sat1 : p.sat0);
    const uint32_t *satz_chip = reinterpret_cast<const uint32_t *>(p.swap ? p.satz1 : p.satz0);
    const uint32_t *satz_win = reinterpret_cast<const uint32_t *>(p.swap ? p.satz0 : p.satz1);
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

    const int chip_nulls = __builtin_amdgcn_readfirstlane((int)sat_box(satz_chip, p.sat_ws, cu0, cv0, CW, CW));
    const int win_nulls = __builtin_amdgcn_readfirstlane((int)sat_box(satz_win, p.sat_ws, wu0, wv0, D2, D2));
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
    uint32_t SX;
    unsigned long long SXX;
    chip_sums_u16(sat_chip, p.sat_ws, cu0, cv0, CW, lane, SX, SXX);

    // ---- stage the tiles: window pixels (x, y), x < SW, y < KW, split into the two planes (both waves); the chip planes: zeros ------
    {
        const int NSEG = L.SW / 16, TTASK = L.KW * NSEG;                // (tile rows >= KW and columns >= SW are only ever weighted 0: left as they are)
        const float inv_nseg = 1.0f / (float)NSEG;                      // t / NSEG for t < 2,304, NSEG <= 12: (t + 1/2) / NSEG lies 1 / 24 from an integer
        const int tsh = wu0 & 1;
        const uint32_t *tgb = reinterpret_cast<const uint32_t *>(win_pl + (size_t)wv0 * Wp + (wu0 - tsh));
        // (the tile reaches past the search box, which may end at the plane's last row: the loads are clamped to the plane; what a
        //  clamped load brings only reaches cells outside the search range)
        const uint32_t tlim = (uint32_t)(((size_t)(p.H + 2 * PAD) * (size_t)Wp - ((size_t)wv0 * Wp + (size_t)(wu0 - tsh))) / 2 - 1);
#pragma unroll 1
        for (int t0 = tid; t0 < TTASK; t0 += 2 * NT) {
            uint32_t td[2][9];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int t = t0 + NT * k;
                const bool on = t < TTASK;
                const int y = (int)(((float)t + 0.5f) * inv_nseg), q = t - NSEG * y;
                const uint32_t go = on ? (uint32_t)y * (uint32_t)(Wp >> 1) + 8u * (uint32_t)q : 0u;
#pragma unroll
                for (int j = 0; j < 9; j++) td[k][j] = tgb[min(go + (uint32_t)j, tlim)];
            }
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int t = t0 + NT * k;
                const int y = (int)(((float)t + 0.5f) * inv_nseg), q = t - NSEG * y;
                if (t < TTASK) {
                    uint32_t e[8], h[4], l[4];
#pragma unroll
                    for (int j = 0; j < 8; j++) e[j] = alignb(td[k][j + 1], td[k][j], 2 * tsh);
#pragma unroll
                    for (int j = 0; j < 4; j++) split4(e[2 * j], e[2 * j + 1], h[j], l[j]);
                    *reinterpret_cast<uint4 *>(WTH + y * PW + 16 * q) = make_uint4(h[0], h[1], h[2], h[3]);
                    *reinterpret_cast<uint4 *>(WTL + y * PW + 16 * q) = make_uint4(l[0], l[1], l[2], l[3]);
                }
            }
        }
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < 2 * L.CHB / 16; i += NT) reinterpret_cast<uint4 *>(CHH)[i] = z4;      // (the two planes are neighbours)
    }
    __syncthreads();
    // ---- the chip planes: CW rows, four pixels per dword ------------------------------------------------------------------------------
    {
        const int CTASK = CW * CD;
        const float inv_cd = 1.0f / (float)CD;                          // t / CD for t < 6,601, CD <= 41: (t + 1/2) / CD lies 1 / 82 from an integer
        const int csh = cu0 & 1;
        const uint32_t *cgb = reinterpret_cast<const uint32_t *>(chip_pl + (size_t)cv0 * Wp + (cu0 - csh));
        const uint32_t lastm = L.LASTN >= 4 ? 0xffffffffu : ((1u << (8 * L.LASTN)) - 1u);
#pragma unroll 1
        for (int t0 = tid; t0 < CTASK; t0 += 4 * NT) {
            uint32_t c0[4], c1[4], c2[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = t0 + NT * k;
                const bool on = t < CTASK;
                const int r = (int)(((float)t + 0.5f) * inv_cd), j = t - CD * r;
                const uint32_t go = on ? (uint32_t)r * (uint32_t)(Wp >> 1) + 2u * (uint32_t)j : 0u;
                c0[k] = cgb[go]; c1[k] = cgb[go + 1u]; c2[k] = cgb[go + 2u];     // (the chip lies inside the image: the plane's border holds the read-ahead)
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = t0 + NT * k;
                const int r = (int)(((float)t + 0.5f) * inv_cd), j = t - CD * r;
                if (t < CTASK) {
                    uint32_t h, l;
                    split4(alignb(c1[k], c0[k], 2 * csh), alignb(c2[k], c1[k], 2 * csh), h, l);
                    const uint32_t m = (j == CD - 1) ? lastm : 0xffffffffu;
                    *reinterpret_cast<uint32_t *>(CHH + CH0 + CP * r + 4 * j) = h & m;
                    *reinterpret_cast<uint32_t *>(CHL + CH0 + CP * r + 4 * j) = l & m;
                }
            }
        }
    }
    __syncthreads();

    // lane (n, h) of wave w: cell column s = 16 w + n; byte i of K chunk c <-> window column 16 w + 64 c + 16 h + i
    const int n = lane & 15, h = lane >> 4;
    const int aoff = n * PW + 16 * wave + 16 * h;                       // A operand: tile row r + 16 mt + n
    const int boff = CH0 + 16 * h - n;                                  // B operand: chip-row bytes 64 c + 16 h - n + i
    const uint32_t bsh = (uint32_t)boff & 3u;
    const int boff4 = boff & ~3;
    // the band of ones of the row-box sums (1 where the byte is a window column of the cell's box, i.e. where the Toeplitz row holds a
    // chip pixel; the wave index cancels)
    v4i hb[KCW];
#pragma unroll
    for (int c = 0; c < KCW; c++) hb[c] = band(64 * c + 16 * h, 4, n, CW, 1u);

    // ---- the product surface (and the null correlations): the double-buffered row loop ------------------------------------------------
    const v4i zero4 = {0, 0, 0, 0};
    // accumulators (two 16 x 16 tiles each): HH, LL, SS; masked form, window nulls zb: sum zb ah, sum zb al, sum zb (a^2 planes)';
    // chip nulls za: sum bh za, sum bl za, sum (b^2 planes)' za, and sum zb za
    v4i acch[2] = {zero4, zero4}, accl[2] = {zero4, zero4}, accs[2] = {zero4, zero4};
    v4i azh[2] = {zero4, zero4}, azl[2] = {zero4, zero4}, az0[2] = {zero4, zero4}, az1[2] = {zero4, zero4}, az2[2] = {zero4, zero4};
    v4i ayh[2] = {zero4, zero4}, ayl[2] = {zero4, zero4}, ay0[2] = {zero4, zero4}, ay1[2] = {zero4, zero4}, ay2[2] = {zero4, zero4};
    v4i azz[2] = {zero4, zero4};
    (void)azh; (void)azl; (void)az0; (void)az1; (void)az2; (void)ayh; (void)ayl; (void)ay0; (void)ay1; (void)ay2; (void)azz;
    {
        struct RowOps { v4i ah[2][KCW], al[2][KCW]; uint32_t dh[KCW][5], dl[KCW][5]; };
        auto issue = [&](int r, RowOps &o) __attribute__((always_inline)) {
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int c = 0; c < KCW; c++) {
                    o.ah[m][c] = *reinterpret_cast<const v4i *>(WTH + aoff + (r + 16 * m) * PW + 64 * c);
                    o.al[m][c] = *reinterpret_cast<const v4i *>(WTL + aoff + (r + 16 * m) * PW + 64 * c);
                }
#pragma unroll
            for (int c = 0; c < KCW; c++) {
                const uint32_t *qh = reinterpret_cast<const uint32_t *>(CHH + boff4 + CP * r + 64 * c);
                const uint32_t *ql = reinterpret_cast<const uint32_t *>(CHL + boff4 + CP * r + 64 * c);
#pragma unroll
                for (int k = 0; k < 5; k++) { o.dh[c][k] = qh[k]; o.dl[c][k] = ql[k]; }
            }
        };
        auto consume = [&](const RowOps &o, bool chip_row) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < KCW; c++) {
                v4i bh, bl;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    bh[k] = (int)alignb(o.dh[c][k + 1], o.dh[c][k], bsh);
                    bl[k] = (int)alignb(o.dl[c][k + 1], o.dl[c][k], bsh);
                }
                const v4i bs = addv(bh, bl);
#pragma unroll
                for (int m = 0; m < 2; m++) {
                    acch[m] = mfma(o.ah[m][c], bh, acch[m]);
                    accl[m] = mfma(o.al[m][c], bl, accl[m]);
                    accs[m] = mfma(addv(o.ah[m][c], o.al[m][c]), bs, accs[m]);
                }
                if constexpr (GEN) {
                    if (wn && chip_row) {
                        // the byte planes of a^2 from the Toeplitz row itself, masked by the band: the padding is not a pixel (the zero row
                        // behind the chip is all such bytes, under the band as well: it takes no part)
                        v4i p0, p1, p2;
                        squares(bh, bl, p0, p1, p2);
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t bm = (uint32_t)hb[c][k] * 255u;
                            p0[k] = (int)((uint32_t)p0[k] & bm); p1[k] = (int)((uint32_t)p1[k] & bm); p2[k] = (int)((uint32_t)p2[k] & bm);
                        }
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            const v4i z = null01v(o.ah[m][c], o.al[m][c]);
                            azh[m] = mfma(z, bh, azh[m]); azl[m] = mfma(z, bl, azl[m]);
                            az0[m] = mfma(z, p0, az0[m]); az1[m] = mfma(z, p1, az1[m]); az2[m] = mfma(z, p2, az2[m]);
                        }
                    }
                    if (cn && chip_row) {
                        // (a padding byte is 0 like a null: only the bytes under the band are chip pixels, and the zero row is none)
                        const v4i za = null01v(bh, bl) & hb[c];
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            v4i p0, p1, p2;
                            squares(o.ah[m][c], o.al[m][c], p0, p1, p2);
                            ayh[m] = mfma(o.ah[m][c], za, ayh[m]); ayl[m] = mfma(o.al[m][c], za, ayl[m]);
                            ay0[m] = mfma(p0, za, ay0[m]); ay1[m] = mfma(p1, za, ay1[m]); ay2[m] = mfma(p2, za, ay2[m]);
                            if (wn) azz[m] = mfma(null01v(o.ah[m][c], o.al[m][c]), za, azz[m]);
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

    // ---- window-side box sums of the wave's 32 x 16 cells: sum b, sum b^2 (and the null count) ------------------------------------
    //      row-box sums R[y][s] = sum_{x = s}^{s + CW - 1} q[y][x] by MFMA (A = 16 tile rows, B = the band of ones), then
    //      Box[dy][s] = sum_{y = dy}^{dy + CW - 1} R[y][s] by MFMA (A = the band of ones, B = the byte planes of R, offset form)
    v4i boxb[2], boxz[2] = {zero4, zero4};
    long long boxq[2][4];
    {
        constexpr int MT = max_ntr(KCW), MC = (MT + 3) / 4;
        const int K128 = 128 * CW;
        auto tile_a = [&](int t, v4i (&ah)[KCW], v4i (&al)[KCW]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < KCW; c++) {
                ah[c] = *reinterpret_cast<const v4i *>(WTH + aoff + 16 * t * PW + 64 * c);
                al[c] = *reinterpret_cast<const v4i *>(WTL + aoff + 16 * t * PW + 64 * c);
            }
        };
        // A operand of the vertical sums -- cell row dy = 16 m + n; K slot (h, i) of chunk c <-> tile row y = 64 c + 16 (i >> 2) + 4 h + (i & 3)
        auto vband = [&](int m, int c) __attribute__((always_inline)) -> v4i { return band(64 * c + 4 * h, 16, 16 * m + n, CW, 1u); };
        {   // sum b (and the null count)
            v4i p0[MC], p1[MC], p2[MC], pz[MC];
#pragma unroll
            for (int t = 0; t < 4 * MC; t++) {
                uint32_t q0 = 0, q1 = 0, q2 = 0, qz = 0;
                if (t < MT && t < NTR) {
                    v4i ah[KCW], al[KCW];
                    tile_a(t, ah, al);
                    v4i Rh = zero4, Rl = zero4;
#pragma unroll
                    for (int c = 0; c < KCW; c++) { Rh = mfma(ah[c], hb[c], Rh); Rl = mfma(al[c], hb[c], Rl); }
#pragma unroll
                    for (int i = 0; i < 4; i++) Rl[i] += 64 * Rh[i];
                    uint32_t unused;
                    planes4(Rl, q0, q1, q2, unused);
                    if (GEN && wn) {                          // the row counts of the nulls, <= 161: one plane
                        v4i Z = zero4;
#pragma unroll
                        for (int c = 0; c < KCW; c++) Z = mfma(null01v(ah[c], al[c]), hb[c], Z);
                        uint32_t u1, u2, u3;
                        planes4(Z, qz, u1, u2, u3);
                    }
                }
                p0[t >> 2][t & 3] = (int)q0; p1[t >> 2][t & 3] = (int)q1; p2[t >> 2][t & 3] = (int)q2; pz[t >> 2][t & 3] = (int)qz;
            }
#pragma unroll
            for (int m = 0; m < 2; m++) {
                v4i v0 = zero4, v1 = zero4, v2 = zero4, vz = zero4;
#pragma unroll
                for (int c = 0; c < MC; c++) {
                    if (c < KCV) {
                        const v4i vb = vband(m, c);
                        v0 = mfma(vb, p0[c], v0); v1 = mfma(vb, p1[c], v1); v2 = mfma(vb, p2[c], v2);
                        if (GEN && wn) vz = mfma(vb, pz[c], vz);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    boxb[m][i] = (v0[i] + K128) + 256 * (v1[i] + K128) + 65536 * (v2[i] + K128);
                    if (GEN && wn) boxz[m][i] = vz[i] + K128;
                }
            }
        }
        {   // sum b^2
            v4i p0[MC], p1[MC], p2[MC], p3[MC];
#pragma unroll
            for (int t = 0; t < 4 * MC; t++) {
                uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
                if (t < MT && t < NTR) {
                    v4i ah[KCW], al[KCW];
                    tile_a(t, ah, al);
                    v4i R0 = zero4, R1 = zero4, R2 = zero4;
#pragma unroll
                    for (int c = 0; c < KCW; c++) {
                        v4i s0, s1, s2;
                        squares(ah[c], al[c], s0, s1, s2);
                        R0 = mfma(s0, hb[c], R0); R1 = mfma(s1, hb[c], R1); R2 = mfma(s2, hb[c], R2);
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++)       // (a u32: the row-box sum of q^2 passes 2^31)
                        R0[i] = (int)((uint32_t)(R0[i] + K128) + 256u * (uint32_t)(R1[i] + K128) + 65536u * (uint32_t)(R2[i] + K128));
                    planes4(R0, q0, q1, q2, q3);
                }
                p0[t >> 2][t & 3] = (int)q0; p1[t >> 2][t & 3] = (int)q1; p2[t >> 2][t & 3] = (int)q2; p3[t >> 2][t & 3] = (int)q3;
            }
#pragma unroll
            for (int m = 0; m < 2; m++) {
                v4i v0 = zero4, v1 = zero4, v2 = zero4, v3 = zero4;
#pragma unroll
                for (int c = 0; c < MC; c++) {
                    if (c < KCV) {
                        const v4i vb = vband(m, c);
                        v0 = mfma(vb, p0[c], v0); v1 = mfma(vb, p1[c], v1); v2 = mfma(vb, p2[c], v2); v3 = mfma(vb, p3[c], v3);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
                    boxq[m][i] = (long long)(v0[i] + K128) + 256ll * (v1[i] + K128) + 65536ll * (v2[i] + K128) + 16777216ll * (v3[i] + K128);
            }
        }
    }
    __syncthreads();                                        // the first tile's bytes become the NCC surface

    // ---- NCC of the 8 cells of this lane (:734): exact integer sums, the float kernel's f64 operations (match_full_chip_kernel.hip) ---
    {
        const int sx_col = 16 * wave + n;
        const int Na = chip_nulls;
        constexpr long long kOff3 = 128ll + 256ll * 128 + 65536ll * 128;       // what three offset byte planes owe per counted pixel
        const double dn0 = (double)(NPX - Na), dsx0 = (double)SX, va0 = dn0 * (double)SXX - dsx0 * dsx0;
        auto cell_in = [&](int m, int i, double &dn, double &dsx, double &va, double &sxy, double &dsy, double &dsyy) __attribute__((always_inline)) {
            int sy = boxb[m][i];
            long long syy = boxq[m][i];
            const long long HH = acch[m][i], LL = accl[m][i], SS = accs[m][i];
            sxy = (double)(4096ll * HH + 64ll * (SS - HH - LL) + LL);      // all chip positions: a null is a zero factor
            dn = dn0; dsx = dsx0; va = va0;
            if (GEN && cn) {                                   // chip nulls take window pixels out of sy, syy
                sy -= 64 * ayh[m][i] + ayl[m][i];
                syy -= (long long)ay0[m][i] + 256ll * ay1[m][i] + 65536ll * ay2[m][i] + kOff3 * Na;
            }
            if (GEN && wn) {                                   // window nulls take chip pixels out of n, sx, sxx
                const int nz = boxz[m][i];
                const int ca = 64 * azh[m][i] + azl[m][i];
                const long long caa = (long long)az0[m][i] + 256ll * az1[m][i] + 65536ll * az2[m][i] + kOff3 * nz;
                dn = (double)(NPX - Na - nz + (cn ? azz[m][i] : 0)); dsx = (double)((int)SX - ca);
                va = dn * (double)((long long)SXX - caa) - dsx * dsx;
            }
            dsy = (double)sy; dsyy = (double)syy;
        };
        uint32_t amb = 0u;
#pragma unroll
        for (int ci = 0; ci < 8; ci++) {
            const int m = ci >> 2, i = ci & 3, ry = 16 * m + 4 * h + i;
            double dn, dsx, va, sxy, dsy, dsyy;
            cell_in(m, i, dn, dsx, va, sxy, dsy, dsyy);
            const double num = dn * sxy - dsx * dsy;
            const double P = va * (dn * dsyy - dsy * dsy);
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
                double dn, dsx, va, sxy, dsy, dsyy;
                cell_in(m, i, dn, dsx, va, sxy, dsy, dsyy);
                const double num = dn * sxy - dsx * dsy;
                const double den = mx::ncc_den_exact(va * (dn * dsyy - dsy * dsy));
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
    const int lds = chip_u16_layout(a.ocw).lds;
    if (lds > 60 * 1024) {              // near or beyond the default limit of LDS (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_full_chip_u16<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_full_chip_u16<C>, dim3(nb), dim3(kNT), lds, stream, a);
    return hipGetLastError();
}

template <bool GEN, bool MULTI, bool SURF>
static hipError_t launch_kcw(const MatchU8Args &a, hipStream_t stream)
{
    switch (chip_u16_layout(a.ocw).KCW) {
    case 1: return launch_one<Cfg<1, GEN, MULTI, SURF>>(a, stream);
    case 2: return launch_one<Cfg<2, GEN, MULTI, SURF>>(a, stream);
    case 3: return launch_one<Cfg<3, GEN, MULTI, SURF>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

template <bool GEN>
static hipError_t launch_kcw_acc(const MatchU8Args &a, hipStream_t stream)
{
    switch (chip_u16_layout(a.ocw).KCW) {
    case 1: return launch_one<AccCfg<1, GEN>>(a, stream);
    case 2: return launch_one<AccCfg<2, GEN>>(a, stream);
    case 3: return launch_one<AccCfg<3, GEN>>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

template <bool GEN>
static hipError_t launch_kcw_peak(const MatchU8Args &a, hipStream_t stream)
{
    switch (chip_u16_layout(a.ocw).KCW) {
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

}  // namespace fchip16

bool full_chip_u16_layout(int ocw, int out[4])
{
    if (ocw < 1 || ocw > kFullChipMaxOcw) return false;
    const fchip16::Layout l = fchip16::chip_u16_layout(ocw);
    out[0] = l.KCW; out[1] = l.NTR; out[2] = l.KCV; out[3] = l.lds;
    return true;
}

hipError_t launch_match_full_chip_u16(MatchU8Args a, int forms, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || !a.mx_flags || !a.sat0 || !a.sat1 || !a.satz0 || !a.satz1 || a.full_R < 1 || a.full_R > 15 ||
        a.ocw < 1 || a.ocw > kFullChipMaxOcw || (a.Wp & 3))
        return hipErrorInvalidValue;
    a.point_flags = nullptr;
    if (forms & kFormsAcc) {            // the stack's planes in the list-mode slots; nothing else is written
        if (!a.stk_sum || !a.stk_cnt || !a.stk_lay || a.out || a.full_cand || a.full_surf || a.full_peak) return hipErrorInvalidValue;
        if (a.stk_shift && !mx::stack_acc_scaled_ok(a)) return hipErrorInvalidValue;
        return fchip16::launch_forms_acc(a, forms, stream);
    }
    if (a.full_peak) {                  // the arg-max cells: with the record alone
        if (a.full_cand || a.full_surf) return hipErrorInvalidValue;
        return fchip16::launch_forms_peak(a, forms, stream);
    }
    if (a.full_cand) {
        if (a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks) return hipErrorInvalidValue;
        return a.full_surf ? fchip16::launch_forms<true, true>(a, forms, stream) : fchip16::launch_forms<true, false>(a, forms, stream);
    }
    return a.full_surf ? fchip16::launch_forms<false, true>(a, forms, stream) : fchip16::launch_forms<false, false>(a, forms, stream);
}

}  // namespace mimc3
