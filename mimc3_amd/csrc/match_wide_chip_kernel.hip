// match_wide_chip_kernel.hip -- exhaustive-search NCC offsets beyond +-15 px for gfx950 at ANY chip half-width 1 <= ocw <= 80, on the
// zero-bordered f32 planes of ANY pair (mimc3_match_ncc_wide_chip): 16-bit DN, float pixels, NaN or negative nulls.  ocw and R (16 .. 47)
// are RUN-TIME values.
//
// The definition is mimc3_match_ncc_full_any's in mode 1, word for word, as match_wide_kernel.hip and match_full_chip_kernel.hip state it:
// every sum is the f64 sum of exactly the reference's terms (MIMC_module.c:723-730), the f32 products widened, ADDITIONS ONLY (no running
// sum that subtracts, no table, no float atomics); both null rules of the reference (validity counts p < MIN_DN in double, a NaN NOT
// counted; inclusion a >= MIN_DN && b >= MIN_DN, a NaN excluded); an excluded pixel staged as the canonical 0.0f; the finish with the
// reference's f64 operations (mx::ncc_den_exact, mx::ncc_quot_exact); the tails of match_wide_kernel.hip.
//
// It is match_full_chip_kernel.hip's band loop run once per CELL TILE of match_wide_u8_kernel.hip's grid:
//   layout   one workgroup of four wave64 = one grid point, XCD-contiguous point order.  The surface of S = 2R + 1 <= 95 cells per side is
//            NTX x NTX tiles of 32 x 32 cells, NTX = ceil(S / 32) <= 3.  LDS: a band (box rows of pitch PB, then chip rows of pitch CWP)
//            and behind it the surface of S rows at pitch 96 words with bytes of its own (it outlives the tiles).  wide_chip_layout(ocw, R)
//            is the ONE constexpr expression of it: kernel, launch, static checks and mimc3_wide_chip_layout all come there.
//   counts   the validity counts of the chip and of the D2 x D2 box (D2 = CW + 2R) are taken in ONE pass of their own in front of the
//            tile loop, read from the planes, every pixel once; -3 is decided there, before any tile work.
//   tiles    tile (tx, ty) holds the cells (32 tx + x, 32 ty + y), 0 <= x, y < 32: 256 tasks of one surface row and four neighbouring
//            cells, ONE per thread (y = tid / 8, x0 = 4 (tid % 8)) -- no slices, no shuffle tree.  A task whose first cell lies beyond S
//            idles; a cell beyond S of a live task is computed (from zeros where its window leaves the box) and dropped.
//   bands    per tile the chip is walked in bands of h <= BR chip rows r0 .. r0 + h - 1: staged are those chip rows and the h + 31 box
//            rows 32 ty + r0 .. 32 ty + r0 + h + 30 over the tile's window columns 32 tx .. 32 tx + CW + 30.  The f64 accumulators stay
//            in registers across the bands of a tile; the four cells are finished after the last band.
//   bodies   the band's excluded pixels (its chip rows, and the box pixels of its window that lie INSIDE the box) choose the body, a
//            workgroup-uniform branch: clean (shared core and six edge sums, the chip sums of the band from one reduction) or masked
//            (six sums under the explicit mask) -- the bodies of match_full_chip_kernel.hip, copied.
//   no read outside the box   staging forms a load address only for a pixel (bx, by) with bx < D2 and by < D2 in BOX coordinates (the
//            two guards of stage_band below); everything else of a band's window is staged as 0.0f and counted nowhere.  The host checks
//            that the box lies inside the planes' border, the kernel checks it again for the _dev entry: a tile's overhang of up to 31
//            columns and rows beyond the box (S = 33, 65) is never read.
// The order of the additions is a function of (ocw, R) and of which body runs in which (tile, band) alone: bands in ascending order, a
// band's rows in ascending order, then the sums of the two bodies.  It does not depend on N, on the point's place in the grid or on
// timing.  On integer-class pixels every partial sum is an exact integer (times a power of two) while m * (largest f32 product) < 2^53,
// m <= 25,921 -- 8-, 12- and 16-bit DN at every ocw -- and the bytes are those of the reference-order sums whatever the bands and bodies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "match_full_tail.h"
#include "match_wide_tail.h"

namespace mimc3 {

namespace wchip {

constexpr int kNT = 256;
constexpr int kVP = 96;                             // pitch (words) of the NCC surface: S <= 95
constexpr int kRMin = 16, kRMax = 47;
constexpr int kTile = 32;                           // cells per tile side
constexpr int kStaticBytes = 4 * 2 * 8 + 4 * 4 * 4; // red_d, red_i below
constexpr int kCuLds = 160 * 1024;
constexpr int kHalfBudget = 79 * 1024;              // two workgroups per CU, their static slots included (kChipLdsBudget's figure)
constexpr int kWholeBudget = kCuLds - kStaticBytes;

template <bool MULTI_>
struct Cfg {                                        // (what match_full_tail.h and match_wide_tail.h ask of a configuration)
    static constexpr bool PEAK = false, MULTI = MULTI_;
    static constexpr int VP = kVP, NT = kNT;
};

struct Layout {
    int CW, CWP, NCH, PB, KW, S, NTX, BR, NB, surf, off_chip, off_val, lds, wgs;
};

// the one expression of the layout
__host__ __device__ constexpr Layout wide_chip_layout(int ocw, int R)
{
    Layout l{};
    l.CW = 2 * ocw + 1;
    l.CWP = (l.CW + 3) & ~3;
    l.NCH = l.CWP / 4;
    const int BW = l.CWP + 32;                      // box pixels a tile row's tasks read: x0 <= 28, + the chunk read ahead
    l.PB = ((BW / 4) & 1) ? BW : BW + 4;            // an odd number of 16-byte slots
    l.KW = l.CW + kTile - 1;                        // window columns (and rows) the 32 x 32 cells of a tile reach
    l.S = 2 * R + 1;
    l.NTX = (l.S + kTile - 1) / kTile;
    l.surf = (l.S * kVP * 4 + 15) & ~15;
    const int row = 4 * (l.PB + l.CWP), fixed = 4 * (kTile - 1) * l.PB;
    // two workgroups per CU where the whole chip is then one band; else one workgroup and the tallest band that fits (a band of h rows
    // restages h + 31 box rows)
    const bool two = fixed + l.CW * row + l.surf <= kHalfBudget;
    const int br = ((two ? kHalfBudget : kWholeBudget) - l.surf - fixed) / row;
    l.BR = br < l.CW ? br : l.CW;
    l.NB = l.BR > 0 ? (l.CW + l.BR - 1) / l.BR : 0;
    l.off_chip = 4 * (l.BR + kTile - 1) * l.PB;
    l.off_val = (l.off_chip + 4 * l.BR * l.CWP + 15) & ~15;
    l.lds = l.off_val + l.surf;
    const int w = kCuLds / (l.lds + kStaticBytes);
    l.wgs = w > 8 ? 8 : w;                          // (32 waves a CU: eight workgroups of four)
    return l;
}

constexpr bool layouts_fit()
{
    for (int ocw = 1; ocw <= kFullChipMaxOcw; ocw++)
        for (int R = kRMin; R <= kRMax; R++) {
            const Layout l = wide_chip_layout(ocw, R);
            if (l.BR < 1 || l.BR > l.CW || l.NB * l.BR < l.CW || l.lds + kStaticBytes > kCuLds || l.wgs < 1) return false;
            if (l.BR == l.CW && l.NB != 1) return false;
            if (l.NTX < 2 || l.NTX > 3 || kTile * l.NTX < l.S) return false;
            // a task reads box pixels x0 .. x0 + CWP + 3 <= 28 + CWP + 3 < PB of rows y + r <= 31 + BR - 1; the bit plane of the candidate
            // tail takes the band's bytes
            if (28 + l.CWP + 4 > l.PB || l.KW > l.PB || l.off_chip < mx::kWideLmBytes || l.CW + 2 * R > 255) return false;
        }
    return true;
}
static_assert(layouts_fit(), "every (ocw 1..80, R 16..47) has a band of one row at least and fits a CU's LDS");
static_assert(2 * kRMax + 1 < kVP, "the surface pitch");
static_assert((2 * kRMax + 1) * (2 * kRMax + 1) <= 64 * 32 * mx::kWideLmWords, "the bit plane of the candidate tail");

constexpr double kMinDn = 1e-10;        // MIN_DN (MIMC_module.c:21), compared in double as there

// ---- the row bodies of match_full_chip_kernel.hip, copied (that file stays as it is) ---------------------------------------------------
// the clean body's accumulators of one task: the product streams of its four cells, the shared core and the six edges of the box sums
struct Clean {
    double sxy[4], core, core2, e[6], e2[6];
};

// one 4-pixel chunk of a chip row against the task's window: A the chip pixels 4c .. 4c + 3, W the window pixels 4c .. 4c + 7.
// FIRST: c == 0 (pixels 0, 1, 2 are edges); LAST: c == NCH - 1, where D = CWP - CW chip pixels are padding and the pixels from CW on
// are edges 3 .. 5, the rest of them in the chunk read ahead.  (The chip's padding takes no part: 0 times an Inf would be a NaN.)
template <bool FIRST, bool LAST, int D>
__device__ __forceinline__ void clean_chunk(Clean &s, const float4 A4, const float4 wa, const float4 wb)
{
    const float A[4] = {A4.x, A4.y, A4.z, A4.w};
    const float W[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool edge_hi = LAST && k >= 4 - D;
        if (!edge_hi) {
#pragma unroll
            for (int i = 0; i < 4; i++) s.sxy[i] += (double)(A[k] * W[k + i]);      // the reference's f32 product, widened
        }
        const float b = W[k];
        if (edge_hi) { s.e[3 + k - (4 - D)] += (double)b; s.e2[3 + k - (4 - D)] += (double)(b * b); }
        else if (FIRST && k < 3) { s.e[k] += (double)b; s.e2[k] += (double)(b * b); }
        else { s.core += (double)b; s.core2 += (double)(b * b); }
    }
    if (LAST) {
#pragma unroll
        for (int k = 0; k < 4; k++)                 // the chunk read ahead: pixels CWP + k = CW + D + k
            if (3 + D + k < 6) { s.e[3 + D + k] += (double)W[4 + k]; s.e2[3 + D + k] += (double)(W[4 + k] * W[4 + k]); }
    }
}

template <int D>
__device__ __forceinline__ void clean_row(Clean &s, const float4 *crow, const float4 *wrow, int NCH)
{
    float4 wa = wrow[0], wb = wrow[1];
    if (NCH == 1) { clean_chunk<true, true, D>(s, crow[0], wa, wb); return; }
    clean_chunk<true, false, D>(s, crow[0], wa, wb);
    wa = wb;
    for (int c = 1; c < NCH - 1; c++) {
        wb = wrow[c + 1];
        clean_chunk<false, false, D>(s, crow[c], wa, wb);
        wa = wb;
    }
    wb = wrow[NCH];
    clean_chunk<false, true, D>(s, crow[NCH - 1], wa, wb);
}

template <class C>
__global__ __launch_bounds__(kNT) void match_ncc_wide_chip(MatchU8Args p, float *surf)
{
    constexpr int VP = C::VP, NT = kNT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red_d[4][2];
    __shared__ int red_i[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int gidx = blockIdx.x;
    {
        const int nb = gridDim.x, per = nb >> 3;
        if (per > 0 && gidx < per * 8) gidx = (gidx & 7) * per + (gidx >> 3);   // XCD-contiguous point order
    }
    if (gidx >= p.N) return;
    const float *chip_pl = reinterpret_cast<const float *>(p.swap ? p.p1 : p.p0);
    const float *win_pl = reinterpret_cast<const float *>(p.swap ? p.p0 : p.p1);
    const int Wp = p.Wp, PAD = p.pad, OCW = p.ocw;
    const int R = p.full_R, S = 2 * R + 1, NC = S * S;
    const Layout L = wide_chip_layout(OCW, R);
    const int CW = L.CW, CWP = L.CWP, NCH = L.NCH, PB = L.PB, KW = L.KW, BR = L.BR, NTX = L.NTX, D2 = CW + 2 * R;   // the search box is D2 x D2 pixels
    float *sf = surf ? surf + (size_t)gidx * (size_t)NC : nullptr;

    auto no_record = [&](float status) __attribute__((always_inline)) {
        if (tid == 0) { mx::full_store(p.out + 8 * (size_t)gidx, status); mx::full_cand_fill<C>(p, gidx, status); }
        if (sf) for (int k = tid; k < NC; k += NT) sf[k] = __builtin_nanf("");
    };
    const double *row = p.xyuvav + (size_t)p.xy_stride * (size_t)gidx + p.xy_col;
    const int u0 = (int)row[0], v0 = (int)row[1];
    // (a point that breaks the bounds the host entry refuses -- only the _dev entry can pass one: no read, all NaN)
    if (u0 - OCW < 0 || u0 + OCW >= p.W || v0 - OCW < 0 || v0 + OCW >= p.H) { no_record(__builtin_nanf("")); return; }
    const int lu = p.full_shift ? p.full_shift[2 * (size_t)gidx] : 0, lv = p.full_shift ? p.full_shift[2 * (size_t)gidx + 1] : 0;
    const int cu0 = u0 - OCW + PAD, cv0 = v0 - OCW + PAD;               // plane position of chip pixel (0, 0)
    const int wu0 = u0 + p.off_u + lu - R - OCW + PAD, wv0 = v0 + p.off_v + lv - R - OCW + PAD;      // ... of box pixel (0, 0)
    if (wu0 < 0 || wv0 < 0 || wu0 + D2 > p.W + 2 * PAD || wv0 + D2 > p.H + 2 * PAD) { no_record(__builtin_nanf("")); return; }

    float *BOX = reinterpret_cast<float *>(smem);
    float *CHIP = reinterpret_cast<float *>(smem + L.off_chip);
    float *val = reinterpret_cast<float *>(smem + L.off_val);
    const float *g0 = win_pl + (size_t)wv0 * Wp + wu0;      // box pixel (0, 0): every box load below is g0[by * Wp + bx], bx, by < D2
    const float *c0 = chip_pl + (size_t)cv0 * Wp + cu0;     // chip pixel (0, 0): every chip load is c0[r * Wp + j], r, j < CW

    // ---- the validity counts, every pixel of chip and box once, from the planes; -3 before any tile work -------------------------------
    {
        int c_lt = 0, b_lt = 0;
        for (int by = wave; by < D2; by += 4)
            for (int bx = lane; bx < D2; bx += 64) b_lt += ((double)g0[(size_t)by * Wp + bx] < kMinDn) ? 1 : 0;
        for (int r = wave; r < CW; r += 4)
            for (int j = lane; j < CW; j += 64) c_lt += ((double)c0[(size_t)r * Wp + j] < kMinDn) ? 1 : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { c_lt += __shfl_xor(c_lt, o, 64); b_lt += __shfl_xor(b_lt, o, 64); }
        if (lane == 0) { red_i[wave][0] = c_lt; red_i[wave][1] = b_lt; }
        __syncthreads();
        c_lt = red_i[0][0] + red_i[1][0] + red_i[2][0] + red_i[3][0];
        b_lt = red_i[0][1] + red_i[1][1] + red_i[2][1] + red_i[3][1];
        __syncthreads();                                    // (the slots are written again by the first band)
        const float max_ratio = 0.8f;
        const float rc = (float)c_lt / (float)(CW * CW);
        const float rw = (float)b_lt / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }

    // ---- the task of this thread in every tile: tile row y, cells x0 .. x0 + 3 ---------------------------------------------------------
    const int y = tid >> 3, x0 = 4 * (tid & 7);
    const bool d1 = CWP - CW == 1;

    for (int ty = 0; ty < NTX; ty++)
        for (int tx = 0; tx < NTX; tx++) {
            const int ox = kTile * tx, oy = kTile * ty;     // the tile's first cell = the box position of its window
            const bool active = ox + x0 < S && oy + y < S;

            Clean cl;
            double sxy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0}, syy[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
            int cn[4] = {0, 0, 0, 0};
            cl.core = cl.core2 = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) cl.sxy[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) cl.e[i] = cl.e2[i] = 0.0;
            int clean_rows = 0;                 // chip rows of the tile's clean bands
            double csx = 0.0, csxx = 0.0;       // ... and their chip sums

            for (int r0 = 0; r0 < CW; r0 += BR) {
                const int h = (CW - r0 < BR) ? CW - r0 : BR;
                // ---- stage the band: canonical null for every excluded pixel, which are counted; the band's chip sums -----------------
                int ex = 0;
                double bsx = 0.0, bsxx = 0.0;
                for (int yy = wave; yy < h + kTile - 1; yy += 4) {
                    const int by = oy + r0 + yy;                        // box row
                    const bool row_in = by < D2;
                    const float *g = g0 + (size_t)(row_in ? by : 0) * Wp;
                    float *dst = BOX + yy * PB;
                    for (int j = lane; j < PB; j += 64) {
                        const int bx = ox + j;                          // box column
                        float v = 0.0f;
                        if (row_in && j < KW && bx < D2) {              // inside the tile's window AND inside the box: the only loads
                            v = g[bx];
                            if (!((double)v >= kMinDn)) { ex++; v = 0.0f; }
                        }
                        dst[j] = v;
                    }
                }
                for (int yy = wave; yy < h; yy += 4) {
                    const float *g = c0 + (size_t)(r0 + yy) * Wp;
                    float *dst = CHIP + yy * CWP;
                    for (int j = lane; j < CWP; j += 64) {
                        float v = 0.0f;
                        if (j < CW) {
                            v = g[j];
                            const double d = (double)v;
                            if (!(d >= kMinDn)) { ex++; v = 0.0f; }
                            else { bsx += d; bsxx += (double)(v * v); }
                        }
                        dst[j] = v;
                    }
                }
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    ex += __shfl_xor(ex, o, 64);
                    bsx += __shfl_xor(bsx, o, 64); bsxx += __shfl_xor(bsxx, o, 64);
                }
                if (lane == 0) { red_i[wave][0] = ex; red_d[wave][0] = bsx; red_d[wave][1] = bsxx; }
                __syncthreads();
                ex = red_i[0][0] + red_i[1][0] + red_i[2][0] + red_i[3][0];
                const bool dirty = ex != 0;                         // workgroup-uniform
                const int rows = active ? h : 0;
                if (!dirty) {
                    csx += (red_d[0][0] + red_d[1][0]) + (red_d[2][0] + red_d[3][0]);
                    csxx += (red_d[0][1] + red_d[1][1]) + (red_d[2][1] + red_d[3][1]);
                    clean_rows += h;
                    for (int r = 0; r < rows; r++) {
                        const float4 *crow = reinterpret_cast<const float4 *>(CHIP + r * CWP);
                        const float4 *wrow = reinterpret_cast<const float4 *>(BOX + (y + r) * PB + x0);
                        if (d1) clean_row<1>(cl, crow, wrow, NCH);
                        else clean_row<3>(cl, crow, wrow, NCH);
                    }
                } else {
                    for (int r = 0; r < rows; r++) {
                        const float4 *crow = reinterpret_cast<const float4 *>(CHIP + r * CWP);
                        const float4 *wrow = reinterpret_cast<const float4 *>(BOX + (y + r) * PB + x0);
                        float4 wa = wrow[0];
#pragma unroll 1
                        for (int c = 0; c < NCH; c++) {
                            const float4 A4 = crow[c], wb = wrow[c + 1];
                            const float A[4] = {A4.x, A4.y, A4.z, A4.w};
                            const float W[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                            for (int k = 0; k < 4; k++)
#pragma unroll
                                for (int i = 0; i < 4; i++) {
                                    const float a = A[k], b = W[k + i];
                                    const bool m = a != 0.0f && b != 0.0f;          // both included (the chip's padding is 0 as well)
                                    cn[i] += m ? 1 : 0;
                                    sx[i] += (double)(m ? a : 0.0f); sy[i] += (double)(m ? b : 0.0f);
                                    sxx[i] += (double)(m ? a * a : 0.0f); syy[i] += (double)(m ? b * b : 0.0f);
                                    sxy[i] += (double)(m ? a * b : 0.0f);
                                }
                            wa = wb;
                        }
                    }
                }
                __syncthreads();                                    // the band's bytes are free: the next band, the next tile, the bit plane
            }

            // ---- NCC of this task's cells (:734): the two bodies' sums, then the reference's f64 operations one by one ----------------
            if (active) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int x = ox + x0 + i;
                    if (x >= S) continue;                           // computed and dropped
                    const double dsxy = sxy[i] + cl.sxy[i];
                    const double dsy = sy[i] + (((cl.core + cl.e[i]) + cl.e[i + 1]) + cl.e[i + 2]);
                    const double dsyy = syy[i] + (((cl.core2 + cl.e2[i]) + cl.e2[i + 1]) + cl.e2[i + 2]);
                    const double dn = (double)(cn[i] + CW * clean_rows);
                    const double dsx = sx[i] + csx, dsxx = sxx[i] + csxx;
                    const double va = dn * dsxx - dsx * dsx;
                    const double num = dn * dsxy - dsx * dsy;
                    const double P = va * (dn * dsyy - dsy * dsy);
                    val[(oy + y) * VP + x] = mx::ncc_quot_exact(num, mx::ncc_den_exact(P));
                }
            }
        }
    __syncthreads();                                        // the surface is complete; the band buffer is dead
    if (sf)
        for (int k = tid; k < NC; k += NT) {
            const int x = k / S, yy = k - S * x;
            sf[k] = val[yy * VP + x];
        }
    uint32_t *bits = reinterpret_cast<uint32_t *>(smem);    // (the band's bytes)
    if constexpr (C::MULTI) {
        mx::wide_lm_plane<C>(p, val, bits, tid);
        __syncthreads();
    }
    if (wave != 0) return;
    mx::full_tail<C>(p, val, gidx, lu, lv, lane);
    if constexpr (C::MULTI) mx::wide_tail_multi<C>(p, val, bits, gidx, lu, lv, lane);
}

template <class C>
static hipError_t launch_one(const MatchU8Args &a, float *surf, hipStream_t stream)
{
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    const int lds = wide_chip_layout(a.ocw, a.full_R).lds;
    if (lds + kStaticBytes > kCuLds) return hipErrorInvalidValue;          // (never: layouts_fit)
    if (lds > 60 * 1024) {              // near or beyond the default limit of LDS, the static slots included (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_wide_chip<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_wide_chip<C>, dim3(nb), dim3(kNT), lds, stream, a, surf);
    return hipGetLastError();
}

}  // namespace wchip

int wide_chip_max_radius(int ocw) { return ocw >= 1 && ocw <= kFullChipMaxOcw ? wchip::kRMax : 0; }

bool wide_chip_layout_query(int ocw, int R, int out[5])
{
    if (ocw < 1 || ocw > kFullChipMaxOcw || R < wchip::kRMin || R > wchip::kRMax) return false;
    const wchip::Layout l = wchip::wide_chip_layout(ocw, R);
    out[0] = l.NTX; out[1] = l.BR; out[2] = l.NB; out[3] = l.wgs; out[4] = l.lds;
    return true;
}

hipError_t launch_match_wide_chip(MatchU8Args a, float *surf, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || a.full_peak || a.ocw < 1 || a.ocw > kFullChipMaxOcw || a.full_R < wchip::kRMin || a.full_R > wchip::kRMax)
        return hipErrorInvalidValue;
    if (a.full_cand && (a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks)) return hipErrorInvalidValue;
    if (a.full_cand) return wchip::launch_one<wchip::Cfg<true>>(a, surf, stream);
    return wchip::launch_one<wchip::Cfg<false>>(a, surf, stream);
}

}  // namespace mimc3
