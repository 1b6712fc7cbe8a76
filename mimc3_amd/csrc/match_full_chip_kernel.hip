// match_full_chip_kernel.hip -- exhaustive-search NCC offsets for gfx950 at ANY chip half-width 1 <= ocw <= 80 (mimc3_match_ncc_full_chip):
// the reference's other chip sets (7, 10, 15, 11 and 14, 30, 60, 80) and everything between.  ocw is a RUN-TIME value here.
//
// Same definition, record, candidates and tail as match_full_f32g_kernel.hip (match_full_tail.h, unedited), on the same zero-bordered
// f32 planes: every sum is the f64 sum of exactly the reference's terms (MIMC_module.c:723-730), the f32 products widened, ADDITIONS
// ONLY (no running sum that subtracts, no table, no float atomics), so a sum of m <= 25,921 (161^2) positive terms is within
// (m - 1) 2^-53 < 2.9e-12 (relative) of the exact sum in any order; both null rules of the reference (validity counts p < MIN_DN in
// double, a NaN NOT counted; inclusion a >= MIN_DN && b >= MIN_DN, a NaN excluded); an excluded pixel staged as the canonical 0.0f.
//
// What is new is the LDS scheme: box plus chip are 255 KB at ocw 80, R 15, so the chip is walked in BANDS of chip rows.
//   layout   one workgroup of four wave64 = one grid point, XCD-contiguous point order.  CW = 2 ocw + 1, CWP = CW rounded up to whole
//            4-pixel chunks (CWP - CW is 1 or 3), box row pitch PB = CWP + 32 or + 36 pixels (an odd number of 16-byte slots).  A band
//            of h <= BR chip rows r0 .. r0 + h - 1 holds those chip rows (pitch CWP, zeros behind the chip) and the h + 2R box rows
//            r0 .. r0 + h + 2R - 1 they meet over all surface rows; BR = chip_layout(ocw, R).BR, the largest height whose band fits
//            kChipLdsBudget (79 KB: two workgroups per CU), or CW when the whole chip does -- then there is ONE band and the kernel
//            has the float kernel's shape.  The 2R box rows two bands share are staged again from the plane (L2 hits): no ring, no
//            row copies in LDS, one staging loop for every band.
//   tasks    a task = one surface row y and four neighbouring cells x0 .. x0 + 3 (at most 248 at S = 31), its band rows dealt to 2^k
//            neighbouring lanes (slice, slice + 2^k, ...), f64 accumulators in registers ACROSS the bands; the cells are finished
//            once, after the last band.
//   counts   while staging every thread counts its pixels under the two rules: the validity counts (chip, and every box row the
//            first time it is staged) accumulate over all bands and decide -3 after the last one; the excluded pixels of THIS band's
//            chip rows and box rows (shared rows included) choose the band's body, a workgroup-uniform branch:
//   clean    (no excluded pixel in the band) sxy the product stream; the four cells share the window pixels 3 .. CW - 1 of a row in ONE
//            core accumulator and take the six edge pixels 0, 1, 2, CW, CW + 1, CW + 2 into one sum each; the band's rows add CW to
//            every cell's n and the band's chip sums (one wave reduction, four LDS slots) to every cell's sx, sxx.  The first and the
//            last chunk of a row are written out with their own pixel classes (at CW = 3 they are the same chunk: no core pixel at
//            all, pixel 3 is the edge CW), the chunks between are all core.
//   dirty    six sums under the explicit mask [a != 0][b != 0], n counting mask bits, every term selected by the mask.
//   A point's cell is then   n = cn + CW * (rows of clean bands),  sx = sx_dirty + sx_clean, ...,  sy = sy_dirty + (core + its edges).
// The order of the additions is a function of (ocw, R, npeaks == 0 -- which changes nothing here) and of which body runs in which band
// alone: bands in ascending order, rows of a band by slice, the shuffle tree over the slices, then the sums of the two bodies.  It does
// not depend on N, on the point's place in the grid or on timing.  On integer-class pixels every partial sum is an exact integer
// (times a power of two) while m * (largest f32 product) < 2^53 -- 8-, 12- and 16-bit DN at every ocw: 2^32 * 25,921 < 2^47 -- and the
// bytes are those of the reference-order sums whatever the bands and bodies.
// The surface (pitch 33) takes the chip band's place; surf, when given, is stored from it before the tail runs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "match_full_tail.h"

namespace mimc3 {

namespace fchip {

constexpr int kNT = 256;
constexpr int kVP = 33;                             // pitch (words) of the NCC surface
constexpr int kValBytes = 4 * 32 * kVP;
constexpr int kStaticBytes = 4 * 2 * 8 + 4 * 3 * 4; // red_d, red_i below

template <bool MULTI_>
struct Cfg {                                        // (what match_full_tail.h asks of a configuration)
    static constexpr bool PEAK = false, MULTI = MULTI_;
    static constexpr int VP = kVP;
};
// The record-only form that also leaves the arg-max cell (or -1) in full_peak, where a pyramid's next level takes its search centre from
// (mimc3_match_ncc_pyramid_chip).  A configuration of its own, as PeakCfg of match_full_f32g_kernel.hip: the two Cfg instantiations keep
// their names and code; it sums in the order of Cfg<false>
struct PeakCfg : Cfg<false> {
    static constexpr bool PEAK = true;
};

struct Layout {
    int CW, CWP, NCH, PB, BR, lds;
};

// the one expression of the layout: the launch, the kernel, the static checks and mimc3_full_chip_band_rows all come here
__host__ __device__ constexpr Layout chip_layout(int ocw, int R)
{
    Layout l{};
    l.CW = 2 * ocw + 1;
    l.CWP = (l.CW + 3) & ~3;
    l.NCH = l.CWP / 4;
    const int BW = l.CWP + 32;                      // box pixels a row's tasks read: x0 <= 28, + the chunk read ahead
    l.PB = ((BW / 4) & 1) ? BW : BW + 4;
    const int row = 4 * (l.PB + l.CWP), fixed = 4 * 2 * R * l.PB;
    int br = (kChipLdsBudget - fixed) / row;
    l.BR = br < l.CW ? br : l.CW;
    const int chipb = 4 * l.BR * l.CWP;
    l.lds = (4 * (l.BR + 2 * R) * l.PB + (chipb > kValBytes ? chipb : kValBytes) + 15) & ~15;
    return l;
}

constexpr bool layouts_fit()
{
    for (int ocw = 1; ocw <= kFullChipMaxOcw; ocw++)
        for (int R = 1; R <= 15; R++) {
            const Layout l = chip_layout(ocw, R);
            // (a band of one row at least; a multi-band chip's band is larger than the surface that takes its place; two workgroups a CU)
            if (l.BR < 1 || l.BR > l.CW || 2 * (l.lds + kStaticBytes) > 160 * 1024) return false;
            if (l.BR < l.CW && l.lds > kChipLdsBudget) return false;
            if (4 * (l.BR + 2 * R) * l.PB + kValBytes > l.lds) return false;
        }
    return true;
}
static_assert(layouts_fit(), "every (ocw, R) fits its LDS");
static_assert(chip_layout(kFullChipMaxOcw, 15).lds + kStaticBytes <= 160 * 1024, "the largest launch fits a CU, static slots included");

constexpr double kMinDn = 1e-10;        // MIN_DN (MIMC_module.c:21), compared in double as there

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
__global__ __launch_bounds__(kNT) void match_ncc_full_chip(MatchU8Args p, float *surf)
{
    constexpr int VP = C::VP, NT = kNT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red_d[4][2];
    __shared__ int red_i[4][3];
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
    const Layout L = chip_layout(OCW, R);
    const int CW = L.CW, CWP = L.CWP, NCH = L.NCH, PB = L.PB, BR = L.BR, D2 = CW + 2 * R;     // the search box is D2 x D2 pixels
    float *sf = surf ? surf + (size_t)gidx * (size_t)NC : nullptr;

    auto no_record = [&](float status) __attribute__((always_inline)) {
        if (tid == 0) { mx::full_store(p.out + 8 * (size_t)gidx, status); mx::full_peak_store<C>(p, gidx, -1); mx::full_cand_fill<C>(p, gidx, status); }
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
    float *CHIP = reinterpret_cast<float *>(smem + (size_t)(BR + 2 * R) * PB * 4);
    float *val = CHIP;

    // ---- the tasks: surface row y, cells x0 .. x0 + 3, band rows slice, slice + nsplit, ... -----------------------------------------
    const int NGX = (S + 3) >> 2, ntask = S * NGX;
    int lsplit = 0;
    while (lsplit < 6 && (ntask << (lsplit + 1)) <= NT) lsplit++;
    const int nsplit = 1 << lsplit, slice = tid & (nsplit - 1), task = tid >> lsplit;
    const bool active = task < ntask;
    const int y = active ? task / NGX : 0, x0 = active ? 4 * (task - NGX * (task / NGX)) : 0;
    const bool d1 = CWP - CW == 1;

    Clean cl;
    double sxy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0}, syy[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
    int cn[4] = {0, 0, 0, 0};
    cl.core = cl.core2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) cl.sxy[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) cl.e[i] = cl.e2[i] = 0.0;
    int c_lt = 0, b_lt = 0;             // the validity counts, over all bands
    int clean_rows = 0;                 // chip rows of the clean bands
    double csx = 0.0, csxx = 0.0;       // ... and their chip sums
    bool any_dirty = false;

    const float *g0 = win_pl + (size_t)wv0 * Wp + wu0;
    const float *c0 = chip_pl + (size_t)cv0 * Wp + cu0;
    for (int r0 = 0; r0 < CW; r0 += BR) {
        const int h = (CW - r0 < BR) ? CW - r0 : BR;
        // ---- stage the band: count under the two rules, canonical null for every excluded pixel; the band's chip sums -------------
        int ex = 0, t_clt = 0, t_blt = 0;
        double bsx = 0.0, bsxx = 0.0;
        const int first_new = r0 == 0 ? 0 : r0 + 2 * R;     // box rows below it were counted with the band before
        for (int yy = wave; yy < h + 2 * R; yy += 4) {
            const float *g = g0 + (size_t)(r0 + yy) * Wp;
            float *dst = BOX + yy * PB;
            const bool count = r0 + yy >= first_new;
            for (int j = lane; j < PB; j += 64) {
                float v = 0.0f;
                if (j < D2) {
                    v = g[j];
                    const double d = (double)v;
                    if (count) t_blt += (d < kMinDn) ? 1 : 0;
                    if (!(d >= kMinDn)) { ex++; v = 0.0f; }
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
                    t_clt += (d < kMinDn) ? 1 : 0;
                    if (!(d >= kMinDn)) { ex++; v = 0.0f; }
                    else { bsx += d; bsxx += (double)(v * v); }
                }
                dst[j] = v;
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            ex += __shfl_xor(ex, o, 64); t_clt += __shfl_xor(t_clt, o, 64); t_blt += __shfl_xor(t_blt, o, 64);
            bsx += __shfl_xor(bsx, o, 64); bsxx += __shfl_xor(bsxx, o, 64);
        }
        if (lane == 0) {
            red_i[wave][0] = ex; red_i[wave][1] = t_clt; red_i[wave][2] = t_blt;
            red_d[wave][0] = bsx; red_d[wave][1] = bsxx;
        }
        __syncthreads();
        ex = red_i[0][0] + red_i[1][0] + red_i[2][0] + red_i[3][0];
        c_lt += red_i[0][1] + red_i[1][1] + red_i[2][1] + red_i[3][1];
        b_lt += red_i[0][2] + red_i[1][2] + red_i[2][2] + red_i[3][2];
        const bool dirty = ex != 0;                         // workgroup-uniform
        if (!dirty) {
            csx += (red_d[0][0] + red_d[1][0]) + (red_d[2][0] + red_d[3][0]);
            csxx += (red_d[0][1] + red_d[1][1]) + (red_d[2][1] + red_d[3][1]);
            clean_rows += h;
            for (int r = active ? slice : h; r < h; r += nsplit) {
                const float4 *crow = reinterpret_cast<const float4 *>(CHIP + r * CWP);
                const float4 *wrow = reinterpret_cast<const float4 *>(BOX + (y + r) * PB + x0);
                if (d1) clean_row<1>(cl, crow, wrow, NCH);
                else clean_row<3>(cl, crow, wrow, NCH);
            }
        } else {
            any_dirty = true;
            for (int r = active ? slice : h; r < h; r += nsplit) {
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
        __syncthreads();                                    // the band's bytes are free: the next band, or the NCC surface
    }
    {
        const float max_ratio = 0.8f;
        const float rc = (float)c_lt / (float)(CW * CW);
        const float rw = (float)b_lt / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }
    // the two bodies' sums of this lane, then the slices of a task (neighbouring lanes; idle lanes hold zeros)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        sxy[i] += cl.sxy[i];
        sy[i] += ((cl.core + cl.e[i]) + cl.e[i + 1]) + cl.e[i + 2];
        syy[i] += ((cl.core2 + cl.e2[i]) + cl.e2[i + 1]) + cl.e2[i + 2];
    }
    for (int o = 1; o < nsplit; o <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sxy[i] += __shfl_xor(sxy[i], o, 64);
            sy[i] += __shfl_xor(sy[i], o, 64); syy[i] += __shfl_xor(syy[i], o, 64);
            if (any_dirty) {
                sxx[i] += __shfl_xor(sxx[i], o, 64);
                cn[i] += __shfl_xor(cn[i], o, 64); sx[i] += __shfl_xor(sx[i], o, 64);
            }
        }
    }

    // ---- NCC of this task's cells (:734): the reference's f64 operations one by one ------------------------------------------------
    if (active && slice == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x0 + i;
            if (x >= S) continue;
            const double dn = (double)(cn[i] + CW * clean_rows);
            const double dsx = sx[i] + csx, dsxx = sxx[i] + csxx;
            const double dsy = sy[i], dsyy = syy[i];
            const double va = dn * dsxx - dsx * dsx;
            const double num = dn * sxy[i] - dsx * dsy;
            const double P = va * (dn * dsyy - dsy * dsy);
            val[y * VP + x] = mx::ncc_quot_exact(num, mx::ncc_den_exact(P));
        }
    }
    __syncthreads();
    if (sf)
        for (int k = tid; k < NC; k += NT) {
            const int x = k / S, yy = k - S * x;
            sf[k] = val[yy * VP + x];
        }
    if (wave != 0) return;
    mx::full_tail<C>(p, val, gidx, lu, lv, lane);
    if constexpr (C::MULTI) mx::full_tail_multi<C>(p, val, gidx, lu, lv, lane);
}

template <class C>
static hipError_t launch_one(const MatchU8Args &a, float *surf, hipStream_t stream)
{
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    const int lds = chip_layout(a.ocw, a.full_R).lds;
    if (lds + kStaticBytes > 160 * 1024) return hipErrorInvalidValue;      // (never: layouts_fit)
    if (lds > 60 * 1024) {              // near or beyond the default limit of LDS, the static slots included (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_full_chip<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_full_chip<C>, dim3(nb), dim3(kNT), lds, stream, a, surf);
    return hipGetLastError();
}

}  // namespace fchip

int full_chip_band_rows(int ocw, int R)
{
    if (ocw < 1 || ocw > kFullChipMaxOcw || R < 1 || R > 15) return 0;
    return fchip::chip_layout(ocw, R).BR;
}

hipError_t launch_match_full_chip(MatchU8Args a, float *surf, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || a.full_R < 1 || a.full_R > 15 || a.ocw < 1 || a.ocw > kFullChipMaxOcw) return hipErrorInvalidValue;
    if (a.full_cand && (a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks)) return hipErrorInvalidValue;
    if (a.full_peak && (a.full_cand || surf)) return hipErrorInvalidValue;
    if (a.full_peak) return fchip::launch_one<fchip::PeakCfg>(a, surf, stream);
    if (a.full_cand) return fchip::launch_one<fchip::Cfg<true>>(a, surf, stream);
    return fchip::launch_one<fchip::Cfg<false>>(a, surf, stream);
}

}  // namespace mimc3
