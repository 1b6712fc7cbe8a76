// match_full_f32_kernel.hip -- exhaustive-search NCC offsets for gfx950 on integral-f32 pairs (f32 planes; every pixel times 2^s, s = 0 or
// 3 per image, an integer w in [0, 2^20): 16-bit DN and what GMA_float_conv2 makes of it).
//
// Same contract as match_full_u16_kernel.hip and the full mode of match_mx_kernel.hip, on the planes and the 16-byte tables the DLC
// matcher's PxF32i kernel reads (build_f32, capi.cpp).  The front below builds the complete (2R + 1)^2 surface of a point; the whole tail
// (arg-max, border and validity rules, fit, SNR, Hessian, the K local maxima) is match_full_tail.h, the text the other fronts run.
//
// What is different on this class: the reference's f32 pixel product ROUNDS above 2^24 (MIMC_module.c:726-730; DESIGN T1), and that
// rounding is part of the result.  sxx, syy and sxy are sums of (double)(float)(a * b), not of exact products:
//   * fl(w_a w_b) is an integer below 2^40, a chip has at most 6,561 pixels: every sum, and every partial sum in any order, is an exact
//     integer below 2^53.  The lanes may therefore split a cell's pixels any way and add their f64 partial sums in any order.
//   * the pixels are w / 2^s; a power of two commutes with the rounding of the product (no overflow, no subnormal: w_a w_b >= 1), with
//     every later f64 operation, with the square root (the exponent 2 (sa + sb) is even) and cancels in the division: the kernel
//     multiplies by 2^s when it stages and works on w alone.
//   * n sxy, sx sy and the variance terms are NOT exact in f64 any more (up to 2^13 * 2^53): the finish performs the reference's
//     operations one by one -- two products and a difference for the numerator and for each variance, their product, sqrt, the division
//     (ncc_den_exact / ncc_quot_exact; the library is built without contraction).  ncc_quot_fast was argued for exact inputs and stays off.
// A pixel is null exactly when w == 0 (MIN_DN = 1e-10 lies below 1/8); box pixels outside the image are the planes' zero border.
//
// One workgroup of four wave64 = one grid point.  The search box ((CW + 2R)^2, CW = 2 ocw + 1) and the chip (rows padded with zeros to
// 4-pixel chunks) are staged in LDS as f32 w (dynamic LDS: the box rows a call's R needs; 78 KB at ocw 40, R 15).  A task = one surface
// row y and four neighbouring cells x0 .. x0 + 3 (x0 a multiple of 4: every window read is an aligned 16 bytes); a small search range
// leaves lanes over, so the chip rows of a task are dealt to 2^k neighbouring lanes and summed over them by shuffles.  Per chip row
// and chunk: one 16-byte chip read (a broadcast), one 16-byte window read, 16 products.
//   clean points  (no null in the chip or the box; known from the tables' null fields before any pixel is read): n = CW^2, sx, sxx are
//                 the chip's table query, sy, syy the cell's box query; only sxy is a product stream -- per product v_mul_f32,
//                 v_cvt_f64_f32, v_add_f64 into one f64 accumulator per cell.
//   dirty points  all six sums are masked streams over the same operands, mask [a != 0][b != 0]: the product of two integers >= 1 is
//                 never 0, so n counts the non-zero products; sx adds a' = [b != 0] a, sxx adds fl(a' a), and the mirror image for sy, syy;
//                 sxy needs no mask.  A kernel of its own, launched right behind over all points: each kernel leaves the other's
//                 points after the header.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "sat_kernel.h"
#include "match_full_tail.h"

namespace mimc3 {

namespace ff32 {

template <int OCW_, bool DIRTY_, bool MULTI_>
struct Cfg {
    static constexpr int OCW = OCW_, CW = 2 * OCW_ + 1, NPX = CW * CW;
    static constexpr bool DIRTY = DIRTY_;
    static constexpr bool PEAK = false, MULTI = MULTI_;         // (what match_full_tail.h asks of a configuration)
    static constexpr bool SURF = false;                         // also store the finished surface to full_surf (SurfCfg)
    static constexpr int VP = 33;                               // pitch (words) of the NCC surface
    static constexpr int NT = 256;
    static constexpr int RMAX = 15;
    static constexpr int CWP = (CW + 3) & ~3;                   // chip row pitch (pixels): whole 4-pixel chunks, zeros behind the chip
    static constexpr int NCH = CWP / 4;
    static constexpr int BW = CWP + 32;                         // box pixels a row's tasks read: x0 <= 28, + the last chunk's 8
    // box row pitch (pixels): an odd number of 16-byte slots, so that neighbouring task rows start on different slots of the bank row
    static constexpr int PB = ((BW / 4) & 1) ? BW : BW + 4;
    static constexpr int CHIPB = CW * CWP * 4;
    static constexpr int VALB = 4 * 32 * VP;
    static constexpr int CHB = ((CHIPB > VALB ? CHIPB : VALB) + 15) & ~15;    // the chip; the surface takes its place once the products are summed
    static constexpr int lds_bytes(int R) { return (CW + 2 * R) * PB * 4 + CHB; }
    static_assert(PB >= BW && PB % 4 == 0, "LDS layout");
};

// ... and for a level of the coarse-to-fine search (mimc3_match_ncc_pyramid_dn): the same record, plus every point's arg-max cell k
// (or -1) in full_peak, where the next level's search centre comes from.  (A configuration of its own, as FullPeakCfg of
// match_mx_kernel.hip, and not a fourth parameter of Cfg: the kernels without it keep their names and their code.)
template <int OCW_, bool DIRTY_>
struct PeakCfg : Cfg<OCW_, DIRTY_, false> {
    static constexpr bool PEAK = true;
};

// ... and with the surfaces (mimc3_match_ncc_full_surf, the stack's class layers): the same record and candidates, plus every point's
// finished f32 surface in full_surf, in k order -- all NaN for a point that gets no_record.  A configuration of its own, as PeakCfg
template <int OCW_, bool DIRTY_, bool MULTI_>
struct SurfCfg : Cfg<OCW_, DIRTY_, MULTI_> {
    static constexpr bool SURF = true;
};

template <class C>
__global__ __launch_bounds__(C::NT) void match_ncc_full_f32(MatchU8Args p)
{
    constexpr int OCW = C::OCW, CW = C::CW, NPX = C::NPX, VP = C::VP, NT = C::NT, CWP = C::CWP, NCH = C::NCH, PB = C::PB;
    static_assert(2 * C::lds_bytes(C::RMAX) <= 160 * 1024, "two workgroups per CU at the largest search range");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int gidx = blockIdx.x;
    {
        const int nb = gridDim.x, per = nb >> 3;
        if (per > 0 && gidx < per * 8) gidx = (gidx & 7) * per + (gidx >> 3);   // XCD-contiguous point order
    }
    if (gidx >= p.N) return;
    const float *chip_pl = reinterpret_cast<const float *>(p.swap ? p.p1 : p.p0);
    const float *win_pl = reinterpret_cast<const float *>(p.swap ? p.p0 : p.p1);
    // scale_k = 2^-s_k: the staging multiplies by 2^s_k (exact)
    const float chip_mul = (float)(1.0 / (p.swap ? p.scale1 : p.scale0)), win_mul = (float)(1.0 / (p.swap ? p.scale0 : p.scale1));
    const int Wp = p.Wp, PAD = p.pad, Ws = p.sat_ws;
    const Sat2 *sat_chip = reinterpret_cast<const Sat2 *>(p.swap ? p.sat1 : p.sat0);
    const Sat2 *sat_win = reinterpret_cast<const Sat2 *>(p.swap ? p.sat0 : p.sat1);
    constexpr unsigned long long kSumMask = (1ull << kSatNullShiftF) - 1ull;

    // ---- point header: the refusals, the class and the validity rule of the other fronts ---------------------------------------------
    auto no_record = [&](float status) __attribute__((always_inline)) {
        if (tid == 0) { mx::full_store(p.out + 8 * (size_t)gidx, status); mx::full_peak_store<C>(p, gidx, -1); mx::full_cand_fill<C>(p, gidx, status); }
        if constexpr (C::SURF) {                            // (no surface exists: all NaN, as the float kernel's)
            const int NC = (2 * p.full_R + 1) * (2 * p.full_R + 1);
            float *sf = p.full_surf + (size_t)gidx * (size_t)NC;
            for (int k = tid; k < NC; k += NT) sf[k] = __builtin_nanf("");
        }
    };
    const double *row = p.xyuvav + (size_t)p.xy_stride * (size_t)gidx + p.xy_col;
    const int u0 = (int)row[0], v0 = (int)row[1];
    // (a point that breaks the bounds the host entry refuses -- only the _dev entry can pass one: no read, all NaN.  Every kernel
    //  writes it: the same values)
    if (u0 - OCW < 0 || u0 + OCW >= p.W || v0 - OCW < 0 || v0 + OCW >= p.H) { no_record(__builtin_nanf("")); return; }
    const int lu = p.full_shift ? p.full_shift[2 * (size_t)gidx] : 0, lv = p.full_shift ? p.full_shift[2 * (size_t)gidx + 1] : 0;
    const int R = p.full_R, S = 2 * R + 1, D2 = CW + 2 * R;             // the search box is D2 x D2 pixels
    const int cu0 = u0 - OCW + PAD, cv0 = v0 - OCW + PAD;               // plane position of chip pixel (0, 0)
    const int wu0 = u0 + p.off_u + lu - R - OCW + PAD, wv0 = v0 + p.off_v + lv - R - OCW + PAD;      // ... of box pixel (0, 0)
    if (wu0 < 0 || wv0 < 0 || wu0 + D2 > p.W + 2 * PAD || wv0 + D2 > p.H + 2 * PAD) { no_record(__builtin_nanf("")); return; }
    const Sat2 chipQ = sat_box(sat_chip, Ws, cu0, cv0, CW, CW);
    const int chip_nulls = (int)(chipQ.a >> kSatNullShiftF);
    const int win_nulls = (int)(sat_box(sat_win, Ws, wu0, wv0, D2, D2).a >> kSatNullShiftF);
    if (((chip_nulls | win_nulls) != 0) != C::DIRTY) return;            // the other kernel's point
    if constexpr (C::DIRTY) {
        const float max_ratio = 0.8f;
        const float rc = (float)chip_nulls / (float)NPX;
        const float rw = (float)win_nulls / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }

    float *BOX = reinterpret_cast<float *>(smem);
    float *CHIP = reinterpret_cast<float *>(smem + (size_t)D2 * PB * 4);
    float *val = CHIP;

    // ---- stage the box and the chip as w = pixel * 2^s; zeros behind the box's and the chip's last pixel of a row ----------------------
    {
        const float *g0 = win_pl + (size_t)wv0 * Wp + wu0;
        for (int t = tid; t < D2 * PB; t += NT) {
            const int y = t / PB, j = t - PB * y;
            BOX[t] = j < D2 ? g0[(size_t)y * Wp + j] * win_mul : 0.0f;
        }
        const float *c0 = chip_pl + (size_t)cv0 * Wp + cu0;
        for (int t = tid; t < CW * CWP; t += NT) {
            const int y = t / CWP, j = t - CWP * y;
            CHIP[t] = j < CW ? c0[(size_t)y * Wp + j] * chip_mul : 0.0f;
        }
    }
    __syncthreads();

    // ---- the tasks: surface row y, cells x0 .. x0 + 3, chip rows slice, slice + nsplit, ... ----------------------------------------
    const int NGX = (S + 3) >> 2, ntask = S * NGX;
    int lsplit = 0;
    while (lsplit < 6 && (ntask << (lsplit + 1)) <= NT) lsplit++;
    const int nsplit = 1 << lsplit, slice = tid & (nsplit - 1), task = tid >> lsplit;
    const bool active = task < ntask;
    const int y = active ? task / NGX : 0, x0 = active ? 4 * (task - NGX * (task / NGX)) : 0;
    double sxy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0}, syy[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
    int cn[4] = {0, 0, 0, 0};
    for (int r = active ? slice : CW; r < CW; r += nsplit) {
        const float4 *crow = reinterpret_cast<const float4 *>(CHIP + r * CWP);
        const float4 *wrow = reinterpret_cast<const float4 *>(BOX + (y + r) * PB + x0);
        float4 wa = wrow[0];
        constexpr int UNR = C::DIRTY ? 1 : NCH;             // (the dirty body is six streams: one chunk is code enough)
#pragma unroll UNR
        for (int c = 0; c < NCH; c++) {
            const float4 A4 = crow[c], wb = wrow[c + 1];
            const float A[4] = {A4.x, A4.y, A4.z, A4.w};
            const float W[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};    // window pixels at offsets 0 .. 7 of the chunk
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float a = A[k], b = W[k + i];
                    const float pr = a * b;                         // the reference's f32 product: rounds above 2^24
                    sxy[i] += (double)pr;
                    if constexpr (C::DIRTY) {
                        const float am = (b != 0.0f) ? a : 0.0f, bm = (a != 0.0f) ? b : 0.0f;      // (-0.0 is a null too)
                        cn[i] += (pr != 0.0f) ? 1 : 0;
                        sx[i] += (double)am; sy[i] += (double)bm;
                        sxx[i] += (double)(am * a); syy[i] += (double)(bm * b);
                    }
                }
            wa = wb;
        }
    }
    // the slices of a task sit in neighbouring lanes: every lane of the wave takes part (idle ones hold zeros)
    for (int o = 1; o < nsplit; o <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sxy[i] += __shfl_xor(sxy[i], o, 64);
            if constexpr (C::DIRTY) {
                sxx[i] += __shfl_xor(sxx[i], o, 64); syy[i] += __shfl_xor(syy[i], o, 64);
                cn[i] += __shfl_xor(cn[i], o, 64); sx[i] += __shfl_xor(sx[i], o, 64); sy[i] += __shfl_xor(sy[i], o, 64);
            }
        }
    }
    __syncthreads();                                        // the chip's bytes become the NCC surface

    // ---- NCC of this task's cells (:734): the reference's f64 operations one by one on the (rounded-product) sums ---------------------
    if (active && slice == 0) {
        double dn0 = 0, dsx0 = 0, va0 = 0;
        if constexpr (!C::DIRTY) {
            dn0 = (double)NPX;
            dsx0 = (double)(chipQ.a & kSumMask);
            va0 = dn0 * (double)chipQ.b - dsx0 * dsx0;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x0 + i;
            if (x >= S) continue;                           // (beyond the search range: its box may leave the tables)
            double dn, dsx, va, dsy, dsyy;
            if constexpr (C::DIRTY) {
                dn = (double)cn[i]; dsx = sx[i]; dsy = sy[i]; dsyy = syy[i];
                va = dn * sxx[i] - dsx * dsx;
            } else {
                const Sat2 boxQ = sat_box(sat_win, Ws, wu0 + x, wv0 + y, CW, CW);
                dn = dn0; dsx = dsx0; va = va0;
                dsy = (double)(boxQ.a & kSumMask); dsyy = (double)boxQ.b;
            }
            const double num = dn * sxy[i] - dsx * dsy;
            const double P = va * (dn * dsyy - dsy * dsy);
            val[y * VP + x] = mx::ncc_quot_exact(num, mx::ncc_den_exact(P));
        }
    }
    __syncthreads();
    if constexpr (C::SURF) {                                // the surface in k order (u outer): coalesced stores, LDS reads at stride VP
        float *sf = p.full_surf + (size_t)gidx * (size_t)(S * S);
        for (int k = tid; k < S * S; k += NT) {
            const int x = k / S, yy = k - S * x;
            sf[k] = val[yy * VP + x];
        }
    }
    if (wave != 0) return;
    mx::full_tail<C>(p, val, gidx, lu, lv, lane);
    if constexpr (C::MULTI) mx::full_tail_multi<C>(p, val, gidx, lu, lv, lane);
}

template <class C>
static hipError_t launch_one(const MatchU8Args &a, unsigned nb, hipStream_t stream)
{
    const int lds = C::lds_bytes(a.full_R);
    if (lds > 64 * 1024) {              // beyond the default limit of dynamic LDS (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_full_f32<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_full_f32<C>, dim3(nb), dim3(C::NT), lds, stream, a);
    return hipGetLastError();
}

template <class Clean, class Dirty>
static hipError_t launch_pair(const MatchU8Args &a, hipStream_t stream)
{
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    const hipError_t e = launch_one<Clean>(a, nb, stream);
    if (e != hipSuccess) return e;
    return launch_one<Dirty>(a, nb, stream);
}

// the record alone, with the arg-max cells (PEAK) or with the candidates (MULTI); with full_surf the SURF form of the latter two
template <int OCW>
static hipError_t launch_ocw(const MatchU8Args &a, hipStream_t stream)
{
    if (a.full_surf) {
        if (a.full_cand) return launch_pair<SurfCfg<OCW, false, true>, SurfCfg<OCW, true, true>>(a, stream);
        return launch_pair<SurfCfg<OCW, false, false>, SurfCfg<OCW, true, false>>(a, stream);
    }
    if (a.full_peak) return launch_pair<PeakCfg<OCW, false>, PeakCfg<OCW, true>>(a, stream);
    if (a.full_cand) return launch_pair<Cfg<OCW, false, true>, Cfg<OCW, true, true>>(a, stream);
    return launch_pair<Cfg<OCW, false, false>, Cfg<OCW, true, false>>(a, stream);
}

}  // namespace ff32

hipError_t launch_match_full_f32(MatchU8Args a, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || !a.sat0 || !a.sat1 || a.full_R < 1 || a.full_R > 15 || !(a.scale0 > 0.0) || !(a.scale1 > 0.0)) return hipErrorInvalidValue;
    if (a.full_cand && (a.full_peak || a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks)) return hipErrorInvalidValue;
    if (a.full_surf && a.full_peak) return hipErrorInvalidValue;
    switch (a.ocw) {
    case 7: return ff32::launch_ocw<7>(a, stream);
    case 15: return ff32::launch_ocw<15>(a, stream);
    case 16: return ff32::launch_ocw<16>(a, stream);
    case 30: return ff32::launch_ocw<30>(a, stream);
    case 32: return ff32::launch_ocw<32>(a, stream);
    case 40: return ff32::launch_ocw<40>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mimc3
