// match_full_f32g_kernel.hip -- exhaustive-search NCC offsets for gfx950 on ANY f32 pair: non-integral pixels, NaN and negative nulls
// (mimc3_match_ncc_full_any; SAR amplitude, filtered or radiometrically corrected imagery, GeoTIFFs whose no-data is NaN or -9999).
//
// Same record, candidates and tail as match_full_f32_kernel.hip (match_full_tail.h, unedited), on the zero-bordered f32 planes build_f32
// makes for every pair (the pixels as they are, -0.0 as +0.0; the border 0).  No summed-area tables: those tabulate integers.
//
// What is different on this class: the f64 sums of float terms depend on the order of the additions, so the definition
// (include/mimc3_hip.h) leaves the order to the kernel and bounds what that can do:
//   * every sum is the f64 sum of exactly the reference's terms (MIMC_module.c:723-730): n counts the pairs with a >= MIN_DN and
//     b >= MIN_DN, sx / sy add (double)a / (double)b, sxx / syy / sxy add the f32 products widened;
//   * ADDITIONS ONLY: no running sum that subtracts, no table difference.  Every included term is positive, so a sum of m <= 6,561 terms
//     is within (m - 1) 2^-53 < 7.3e-13 (relative) of the exact sum in any order;
//   * the order is a function of (ocw, R) alone: lanes, slices and the shuffle tree below are fixed, a call is deterministic;
//   * on an integer-class pair every partial sum is an exact integer (times a power of two) below 2^53: the bytes of
//     mimc3_match_ncc_full_dn.
// The two null rules of the reference differ on NaN and both are kept:
//   validity   counts the pixels with p < MIN_DN (compared in double, :622 / :631) in the chip and in the whole box; a NaN is NOT counted;
//   inclusion  a >= MIN_DN && b >= MIN_DN (:723); a NaN IS excluded, as are 0, negatives and positives below 1e-10.
// An excluded pixel is staged as the canonical null 0.0f, so the bodies test != 0 and no NaN reaches an accumulator through an excluded
// pixel; an included Inf, or a product that overflows, goes through the arithmetic as in the reference.
//
// One workgroup of four wave64 = one grid point; box and chip in LDS as f32, a task = one surface row y and four neighbouring cells,
// its chip rows dealt to 2^k neighbouring lanes, f64 accumulators, __shfl_xor reduction -- the layout of match_full_f32_kernel.hip.
// While staging, every thread counts its pixels under the two rules and (chip) adds sx and sxx; one wave reduction and four LDS slots
// per quantity make the point's counts.  The body is then chosen per workgroup (a uniform branch; one launch):
//   clean  (no excluded pixel in chip or box)  n = CW^2; sx, sxx once per point; sxy the product stream (v_mul_f32, v_cvt_f64_f32,
//          v_add_f64).  sy, syy have no table to come from: the task's four cells share the window pixels 3 .. CW - 1 of a row, which go
//          into ONE accumulator, and the six edge pixels 0, 1, 2, CW, CW + 1, CW + 2 into one each -- over all chip rows of the slice;
//          a cell's sum is the core plus its three edge sums.  CW + 3 additions per row for four cells where a stream of its own would
//          take 4 CW, on window values the product stream holds in registers anyway: no LDS intermediate, no extra barrier.
//   dirty  six sums under the explicit mask [a != 0][b != 0]: n counts mask bits (a float product can underflow to 0, so the products
//          are not counted), every term is selected by the mask (0 * Inf must not make a NaN).
// The surface (pitch 33) takes the chip's place; surf, when given, is stored from it before the tail runs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "match_full_tail.h"

namespace mimc3 {

namespace fg32 {

template <int OCW_, bool MULTI_>
struct Cfg {
    static constexpr int OCW = OCW_, CW = 2 * OCW_ + 1, NPX = CW * CW;
    static constexpr bool PEAK = false, MULTI = MULTI_;         // (what match_full_tail.h asks of a configuration)
    static constexpr int VP = 33;                               // pitch (words) of the NCC surface
    static constexpr int NT = 256;
    static constexpr int RMAX = 15;
    static constexpr int CWP = (CW + 3) & ~3;                   // chip row pitch (pixels): whole 4-pixel chunks, zeros behind the chip
    static constexpr int NCH = CWP / 4;
    static constexpr int BW = CWP + 32;                         // box pixels a row's tasks read: x0 <= 28, + the last chunk's 8
    static constexpr int PB = ((BW / 4) & 1) ? BW : BW + 4;     // box row pitch: an odd number of 16-byte slots
    static constexpr int CHIPB = CW * CWP * 4;
    static constexpr int VALB = 4 * 32 * VP;
    static constexpr int CHB = ((CHIPB > VALB ? CHIPB : VALB) + 15) & ~15;    // the chip; the surface takes its place
    static constexpr int lds_bytes(int R) { return (CW + 2 * R) * PB * 4 + CHB; }
    static_assert(PB >= BW && PB % 4 == 0, "LDS layout");
    static_assert(CWP - CW == 1 || CWP - CW == 3, "the edge pixels CW .. CW + 2 sit in the last chunk and the one read ahead");
};

// The record-only form that also leaves the arg-max cell (or -1) in full_peak, where the next level's search centre comes from
// (mimc3_match_ncc_pyramid_any).  A configuration of its own, as PeakCfg of match_full_f32_kernel.hip, not a third parameter of Cfg: the
// existing instantiations keep their names.  It shares every statement of the accumulation with Cfg<OCW, false>: the same sums in the
// same order, so the same surface bits.
template <int OCW_>
struct PeakCfg : Cfg<OCW_, false> {
    static constexpr bool PEAK = true;
};

constexpr double kMinDn = 1e-10;        // MIN_DN (MIMC_module.c:21), compared in double as there

template <class C>
__global__ __launch_bounds__(C::NT) void match_ncc_full_f32g(MatchU8Args p, float *surf)
{
    constexpr int OCW = C::OCW, CW = C::CW, NPX = C::NPX, VP = C::VP, NT = C::NT, CWP = C::CWP, NCH = C::NCH, PB = C::PB;
    static_assert(C::lds_bytes(C::RMAX) <= 160 * 1024, "one workgroup fits a CU at the largest search range");
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
    const int Wp = p.Wp, PAD = p.pad;
    const int R = p.full_R, S = 2 * R + 1, D2 = CW + 2 * R, NC = S * S;    // the search box is D2 x D2 pixels
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
    float *CHIP = reinterpret_cast<float *>(smem + (size_t)D2 * PB * 4);
    float *val = CHIP;

    // ---- stage the box and the chip: count under the two rules, canonical null for every excluded pixel; the chip's sx and sxx ----
    int c_lt = 0, c_ex = 0, b_lt = 0, b_ex = 0;
    double csx = 0.0, csxx = 0.0;
    {
        const float *g0 = win_pl + (size_t)wv0 * Wp + wu0;
        for (int t = tid; t < D2 * PB; t += NT) {
            const int y = t / PB, j = t - PB * y;
            float v = 0.0f;
            if (j < D2) {
                v = g0[(size_t)y * Wp + j];
                const double d = (double)v;
                b_lt += (d < kMinDn) ? 1 : 0;
                if (!(d >= kMinDn)) { b_ex++; v = 0.0f; }
            }
            BOX[t] = v;
        }
        const float *c0 = chip_pl + (size_t)cv0 * Wp + cu0;
        for (int t = tid; t < CW * CWP; t += NT) {
            const int y = t / CWP, j = t - CWP * y;
            float v = 0.0f;
            if (j < CW) {
                v = c0[(size_t)y * Wp + j];
                const double d = (double)v;
                c_lt += (d < kMinDn) ? 1 : 0;
                if (!(d >= kMinDn)) { c_ex++; v = 0.0f; }
                else { csx += d; csxx += (double)(v * v); }
            }
            CHIP[t] = v;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        c_lt += __shfl_xor(c_lt, o, 64); c_ex += __shfl_xor(c_ex, o, 64);
        b_lt += __shfl_xor(b_lt, o, 64); b_ex += __shfl_xor(b_ex, o, 64);
        csx += __shfl_xor(csx, o, 64); csxx += __shfl_xor(csxx, o, 64);
    }
    if (lane == 0) {
        red_i[wave][0] = c_lt; red_i[wave][1] = c_ex; red_i[wave][2] = b_lt; red_i[wave][3] = b_ex;
        red_d[wave][0] = csx; red_d[wave][1] = csxx;
    }
    __syncthreads();
    c_lt = red_i[0][0] + red_i[1][0] + red_i[2][0] + red_i[3][0];
    c_ex = red_i[0][1] + red_i[1][1] + red_i[2][1] + red_i[3][1];
    b_lt = red_i[0][2] + red_i[1][2] + red_i[2][2] + red_i[3][2];
    b_ex = red_i[0][3] + red_i[1][3] + red_i[2][3] + red_i[3][3];
    csx = (red_d[0][0] + red_d[1][0]) + (red_d[2][0] + red_d[3][0]);
    csxx = (red_d[0][1] + red_d[1][1]) + (red_d[2][1] + red_d[3][1]);
    {
        const float max_ratio = 0.8f;
        const float rc = (float)c_lt / (float)NPX;
        const float rw = (float)b_lt / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }
    const bool dirty = (c_ex | b_ex) != 0;                  // workgroup-uniform

    // ---- the tasks: surface row y, cells x0 .. x0 + 3, chip rows slice, slice + nsplit, ... ----------------------------------------
    const int NGX = (S + 3) >> 2, ntask = S * NGX;
    int lsplit = 0;
    while (lsplit < 6 && (ntask << (lsplit + 1)) <= NT) lsplit++;
    const int nsplit = 1 << lsplit, slice = tid & (nsplit - 1), task = tid >> lsplit;
    const bool active = task < ntask;
    const int y = active ? task / NGX : 0, x0 = active ? 4 * (task - NGX * (task / NGX)) : 0;
    double sxy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0}, syy[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
    int cn[4] = {0, 0, 0, 0};
    if (!dirty) {
        double core = 0.0, core2 = 0.0, e[6] = {0, 0, 0, 0, 0, 0}, e2[6] = {0, 0, 0, 0, 0, 0};
        for (int r = active ? slice : CW; r < CW; r += nsplit) {
            const float4 *crow = reinterpret_cast<const float4 *>(CHIP + r * CWP);
            const float4 *wrow = reinterpret_cast<const float4 *>(BOX + (y + r) * PB + x0);
            float4 wa = wrow[0];
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const float4 A4 = crow[c], wb = wrow[c + 1];
                const float A[4] = {A4.x, A4.y, A4.z, A4.w};
                const float W[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};    // window pixels 4c .. 4c + 7 of the task's row
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int q = 4 * c + k;
                    // (the chip's padding takes no part: 0 times an Inf next to the cell would be a NaN)
                    if (q < CW) {
#pragma unroll
                        for (int i = 0; i < 4; i++) sxy[i] += (double)(A[k] * W[k + i]);     // the reference's f32 product, widened
                    }
                    // the box sums: window pixel q = 4c + k once -- the cells' common core or one of the six edges
                    const float b = W[k];
                    if (q < 3) { e[q] += (double)b; e2[q] += (double)(b * b); }
                    else if (q < CW) { core += (double)b; core2 += (double)(b * b); }
                    else if (q < CW + 3) { e[3 + q - CW] += (double)b; e2[3 + q - CW] += (double)(b * b); }
                }
                if (c == NCH - 1) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {           // the chunk read ahead: pixels CWP .. CWP + 3
                        const int q = CWP + k;
                        const float b = W[4 + k];
                        if (q < CW + 3) { e[3 + q - CW] += (double)b; e2[3 + q - CW] += (double)(b * b); }
                    }
                }
                wa = wb;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sy[i] = ((core + e[i]) + e[i + 1]) + e[i + 2];
            syy[i] = ((core2 + e2[i]) + e2[i + 1]) + e2[i + 2];
        }
    } else {
        for (int r = active ? slice : CW; r < CW; r += nsplit) {
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
    // the slices of a task sit in neighbouring lanes: every lane of the wave takes part (idle ones hold zeros)
    for (int o = 1; o < nsplit; o <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sxy[i] += __shfl_xor(sxy[i], o, 64);
            sy[i] += __shfl_xor(sy[i], o, 64); syy[i] += __shfl_xor(syy[i], o, 64);
            if (dirty) {
                sxx[i] += __shfl_xor(sxx[i], o, 64);
                cn[i] += __shfl_xor(cn[i], o, 64); sx[i] += __shfl_xor(sx[i], o, 64);
            }
        }
    }
    __syncthreads();                                        // the chip's bytes become the NCC surface

    // ---- NCC of this task's cells (:734): the reference's f64 operations one by one ------------------------------------------------
    if (active && slice == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x0 + i;
            if (x >= S) continue;
            const double dn = dirty ? (double)cn[i] : (double)NPX;
            const double dsx = dirty ? sx[i] : csx, dsxx = dirty ? sxx[i] : csxx;
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
    const int lds = C::lds_bytes(a.full_R);
    if (lds > 60 * 1024) {              // near or beyond the default limit of LDS, the static slots included (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_full_f32g<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_full_f32g<C>, dim3(nb), dim3(C::NT), lds, stream, a, surf);
    return hipGetLastError();
}

template <int OCW>
static hipError_t launch_ocw(const MatchU8Args &a, float *surf, hipStream_t stream)
{
    if (a.full_peak) return launch_one<PeakCfg<OCW>>(a, surf, stream);
    if (a.full_cand) return launch_one<Cfg<OCW, true>>(a, surf, stream);
    return launch_one<Cfg<OCW, false>>(a, surf, stream);
}

}  // namespace fg32

hipError_t launch_match_full_f32g(MatchU8Args a, float *surf, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || a.full_R < 1 || a.full_R > 15) return hipErrorInvalidValue;
    if (a.full_peak && (a.full_cand || surf)) return hipErrorInvalidValue;
    if (a.full_cand && (a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks)) return hipErrorInvalidValue;
    switch (a.ocw) {
    case 7: return fg32::launch_ocw<7>(a, surf, stream);
    case 15: return fg32::launch_ocw<15>(a, surf, stream);
    case 16: return fg32::launch_ocw<16>(a, surf, stream);
    case 30: return fg32::launch_ocw<30>(a, surf, stream);
    case 32: return fg32::launch_ocw<32>(a, surf, stream);
    case 40: return fg32::launch_ocw<40>(a, surf, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mimc3
