// match_full_u16_kernel.hip -- exhaustive-search NCC offsets for gfx950 on scaled-integer pairs (u16 planes, q = value * 2^s < 4096).
//
// Same contract as the full mode of match_mx_kernel.hip (mimc3_match_ncc_full / _full_multi), on the planes the DLC matcher's PxU16
// kernels read: 12-bit DN, and what GMA_float_conv2 makes of an 8-bit pair (gradients: integers, Laplacian: multiples of 1/8).  The
// front below builds the complete (2R + 1)^2 surface of a point from exact integer sums; the NCC finish of a cell and the whole tail
// (arg-max, border and validity rules, fit, SNR, Hessian, the K local maxima) are match_full_tail.h, the text the 8-bit kernels run.
//
// Why the integers q serve: every f32 product of two pixels q_a / 2^sa * q_b / 2^sb is exact (< 2^24 significant bits), every f64 sum an
// exact integer times a power of two, n sxy - sx sy and both variance terms are exact (< 2^50), and the scale 2^-(sa + sb) commutes with the
// one rounding of the variance product, with the square root (an even exponent) and with the division: the reference's cell on the float
// pixels equals the same formula on q bit for bit.  A pixel is null exactly when q == 0.
//
// One workgroup of four wave64 = one grid point.  The search box ((CW + 2R)^2 u16, CW = 2 ocw + 1) and the chip (rows padded with zeros
// to 8-pixel chunks) are staged in LDS as pixel pairs.  A task = one surface row y and four neighbouring cells x0 .. x0 + 3 (x0 a
// multiple of 4, so the window pairs of the even cells are aligned dwords and those of the odd cells one v_alignbit away); a small
// search range leaves lanes over, so the chip rows of a task are dealt to 2^k neighbouring lanes and summed over them by shuffles.
// Per chip row and chunk: one 16-byte chip read (the same address in every lane of a task row: a broadcast), two 8-byte window reads,
// five v_alignbit and sixteen v_dot2_u32_u16 for 32 products.  A row's partial sums stay below 2^32 (81 * 4095^2) and are added to
// 64-bit accumulators once per row.
//   clean points  (no null in the chip or the box; known from the two null tables before any pixel is read): n = CW^2, sx, sxx are the
//                 chip's table query, sy, syy the cell's box query of the packed table (q | q^2 << 25); only sxy is a product stream.
//   dirty points  all six sums are masked streams over the same operands: with za = [a != 0], zb = [b != 0] as 0 / 1 pairs and their
//                 0xffff masks, n = za . zb, sx = a . zb, sy = za . b, sxy = a . b, sxx = a . (a & mb), syy = b . (b & ma) -- eight
//                 instructions per pixel pair where the clean body has one.  A kernel of its own (its registers do not weigh on the
//                 clean one), launched right behind over all points: each kernel leaves the other's points after the header.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "sat_kernel.h"
#include "match_full_tail.h"

namespace mimc3 {

namespace fu16 {

typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t dot2(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, a), __builtin_bit_cast(us2_t, b), c, false);
}
// the pixel pair that starts at the high half of lo
__device__ __forceinline__ uint32_t odd_pair(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }
// 1 in each half whose pixel is not null (q <= 4095: q + 4095 < 2^13 carries into bit 12 exactly when q >= 1, never into the other half)
__device__ __forceinline__ uint32_t nonnull_pair(uint32_t q) { return ((q + 0x0fff0fffu) >> 12) & 0x00010001u; }

template <int OCW_, bool DIRTY_, bool MULTI_>
struct Cfg {
    static constexpr int OCW = OCW_, CW = 2 * OCW_ + 1, NPX = CW * CW;
    static constexpr bool DIRTY = DIRTY_;
    static constexpr bool PEAK = false, MULTI = MULTI_;         // (what match_full_tail.h asks of a configuration)
    static constexpr bool SURF = false;                         // also store the finished surface to full_surf (SurfCfg)
    static constexpr int VP = 33;                               // pitch (words) of the NCC surface
    static constexpr int NT = 256;
    static constexpr int RMAX = 15, SMAX = 2 * RMAX + 1;
    static constexpr int CWP = (CW + 7) & ~7;                   // chip row pitch (pixels): whole 8-pixel chunks, zeros behind the chip
    static constexpr int NCH = CWP / 8;
    static constexpr int BROWS = CW + 2 * RMAX;                 // box rows
    static constexpr int BW = CWP + 32;                         // box pixels a row's tasks read: x0 <= 28, + the last chunk's 12
    // box row pitch (bytes): 64 mod 128, so that the four task rows of a half-wave's 8-byte reads fall on different banks
    static constexpr int PB = ((2 * BW + 63) & ~127) + 64;
    static constexpr int BOXB = BROWS * PB;
    static constexpr int CHIPB = CW * 2 * CWP;
    static constexpr int VALB = 4 * 32 * VP;
    static constexpr int OFF_CH = BOXB;                         // the chip; the surface takes its place once the products are summed
    static constexpr int LDS = OFF_CH + (((CHIPB > VALB ? CHIPB : VALB) + 15) & ~15);
    static_assert(PB >= 2 * BW && PB % 8 == 0 && LDS <= 65536, "LDS layout");
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
__global__ __launch_bounds__(C::NT) void match_ncc_full_u16(MatchU8Args p)
{
    constexpr int OCW = C::OCW, CW = C::CW, NPX = C::NPX, VP = C::VP, NT = C::NT, CWP = C::CWP, NCH = C::NCH, PB = C::PB;
    __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS];
    uint32_t *BOX = reinterpret_cast<uint32_t *>(smem);
    uint32_t *CHIP = reinterpret_cast<uint32_t *>(smem + C::OFF_CH);
    float *val = reinterpret_cast<float *>(smem + C::OFF_CH);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int gidx = blockIdx.x;
    {
        const int nb = gridDim.x, per = nb >> 3;
        if (per > 0 && gidx < per * 8) gidx = (gidx & 7) * per + (gidx >> 3);   // XCD-contiguous point order
    }
    if (gidx >= p.N) return;
    const unsigned short *chip_pl = reinterpret_cast<const unsigned short *>(p.swap ? p.p1 : p.p0);
    const unsigned short *win_pl = reinterpret_cast<const unsigned short *>(p.swap ? p.p0 : p.p1);
    const int Wp = p.Wp, PAD = p.pad, Ws = p.sat_ws;
    typedef unsigned long long SatT;
    const SatT *sat_chip = reinterpret_cast<const SatT *>(p.swap ? p.sat1 : p.sat0);
    const SatT *sat_win = reinterpret_cast<const SatT *>(p.swap ? p.sat0 : p.sat1);
    const uint32_t *satz_chip = reinterpret_cast<const uint32_t *>(p.swap ? p.satz1 : p.satz0);
    const uint32_t *satz_win = reinterpret_cast<const uint32_t *>(p.swap ? p.satz0 : p.satz1);

    // ---- point header: the refusals, the class and the validity rule of the 8-bit kernels' full mode ---------------------------------
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
    const int chip_nulls = (int)sat_box(satz_chip, Ws, cu0, cv0, CW, CW);
    const int win_nulls = (int)sat_box(satz_win, Ws, wu0, wv0, D2, D2);
    if (((chip_nulls | win_nulls) != 0) != C::DIRTY) return;            // the other kernel's point
    if constexpr (C::DIRTY) {
        const float max_ratio = 0.8f;
        const float rc = (float)chip_nulls / (float)NPX;
        const float rw = (float)win_nulls / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }

    // ---- stage the box and the chip as pixel pairs (aligned dwords of the plane rows, shifted by a pixel where the origin is odd) ---
    {
        constexpr int BD = PB / 4;                                      // dwords per box row
        const int sh = wu0 & 1, nd = (D2 + 1) >> 1;                     // D2 is odd: dword nd - 1 holds the row's last pixel alone
        const uint32_t *g0 = reinterpret_cast<const uint32_t *>(win_pl + (size_t)wv0 * Wp + (wu0 - sh));
        for (int t = tid; t < D2 * BD; t += NT) {
            const int y = t / BD, j = t - BD * y;
            uint32_t w = 0u;
            if (j < nd) {
                const uint32_t *g = g0 + (size_t)y * (size_t)(Wp >> 1) + j;
                const uint32_t d0 = g[0];
                // (origin odd: the pair's second pixel lies in the next dword, read only where the box holds it)
                w = sh ? odd_pair(j < nd - 1 ? g[1] : 0u, d0) : d0;
                if (j == nd - 1) w &= 0xffffu;
            }
            BOX[y * BD + j] = w;
        }
        constexpr int CD = CWP / 2, CN = (CW + 1) >> 1;
        const int csh = cu0 & 1;
        const uint32_t *c0 = reinterpret_cast<const uint32_t *>(chip_pl + (size_t)cv0 * Wp + (cu0 - csh));
        for (int t = tid; t < CW * CD; t += NT) {
            const int y = t / CD, j = t - CD * y;
            uint32_t w = 0u;
            if (j < CN) {
                const uint32_t *g = c0 + (size_t)y * (size_t)(Wp >> 1) + j;
                const uint32_t d0 = g[0];
                w = csh ? odd_pair(j < CN - 1 ? g[1] : 0u, d0) : d0;
                if (j == CN - 1) w &= 0xffffu;
            }
            CHIP[y * CD + j] = w;
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
    unsigned long long sxy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0}, syy[4] = {0, 0, 0, 0};
    uint32_t cn[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
    for (int r = active ? slice : CW; r < CW; r += nsplit) {
        const uint32_t *crow = CHIP + r * (CWP / 2);
        const uint32_t *wrow = BOX + (y + r) * (PB / 4) + (x0 >> 1);
        uint32_t rxy[4] = {0, 0, 0, 0}, rxx[4] = {0, 0, 0, 0}, ryy[4] = {0, 0, 0, 0};
        uint2 wa = *reinterpret_cast<const uint2 *>(wrow);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const uint4 A4 = *reinterpret_cast<const uint4 *>(crow + 4 * c);
            const uint2 wb = *reinterpret_cast<const uint2 *>(wrow + 4 * c + 2), wc = *reinterpret_cast<const uint2 *>(wrow + 4 * c + 4);
            const uint32_t A[4] = {A4.x, A4.y, A4.z, A4.w};
            // window pairs at pixel offsets 0 .. 11 of the chunk: E[j] at 2 j, O[j] at 2 j + 1
            const uint32_t E[6] = {wa.x, wa.y, wb.x, wb.y, wc.x, wc.y};
            uint32_t O[5];
#pragma unroll
            for (int j = 0; j < 5; j++) O[j] = odd_pair(E[j + 1], E[j]);
            if constexpr (!C::DIRTY) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    rxy[0] = dot2(A[k], E[k], rxy[0]);
                    rxy[1] = dot2(A[k], O[k], rxy[1]);
                    rxy[2] = dot2(A[k], E[k + 1], rxy[2]);
                    rxy[3] = dot2(A[k], O[k + 1], rxy[3]);
                }
            } else {
                uint32_t ZA[4], MA[4], ZE[5], ZO[5];
#pragma unroll
                for (int k = 0; k < 4; k++) { ZA[k] = nonnull_pair(A[k]); MA[k] = ZA[k] * 0xffffu; }
#pragma unroll
                for (int j = 0; j < 5; j++) { ZE[j] = nonnull_pair(E[j]); ZO[j] = nonnull_pair(O[j]); }
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int j = k + (i >> 1);
                        const uint32_t B = (i & 1) ? O[j] : E[j], ZB = (i & 1) ? ZO[j] : ZE[j];
                        cn[i] = dot2(ZA[k], ZB, cn[i]);
                        sx[i] = dot2(A[k], ZB, sx[i]);
                        sy[i] = dot2(ZA[k], B, sy[i]);
                        rxy[i] = dot2(A[k], B, rxy[i]);
                        rxx[i] = dot2(A[k], A[k] & (ZB * 0xffffu), rxx[i]);
                        ryy[i] = dot2(B, B & MA[k], ryy[i]);
                    }
            }
            wa = wc;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sxy[i] += rxy[i];
            if constexpr (C::DIRTY) { sxx[i] += rxx[i]; syy[i] += ryy[i]; }
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

    // ---- NCC of this task's cells (:734): exact integer sums, the f64 formula rounded to f32 (match_full_tail.h) -------------------
    if (active && slice == 0) {
        double dn0 = 0, dsx0 = 0, va0 = 0;
        if constexpr (!C::DIRTY) {
            const SatT chipQ = sat_box(sat_chip, Ws, cu0, cv0, CW, CW);
            dn0 = (double)NPX;
            dsx0 = (double)(uint32_t)(chipQ & ((1ull << kSatSqShift16) - 1ull));
            va0 = dn0 * (double)(chipQ >> kSatSqShift16) - dsx0 * dsx0;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x0 + i;
            if (x >= S) continue;                           // (beyond the search range: its box may leave the tables)
            double dn, dsx, va, dsy, dsyy;
            if constexpr (C::DIRTY) {
                dn = (double)cn[i]; dsx = (double)sx[i]; dsy = (double)sy[i]; dsyy = (double)syy[i];
                va = dn * (double)sxx[i] - dsx * dsx;
            } else {
                const SatT boxQ = sat_box(sat_win, Ws, wu0 + x, wv0 + y, CW, CW);
                dn = dn0; dsx = dsx0; va = va0;
                dsy = (double)(uint32_t)(boxQ & ((1ull << kSatSqShift16) - 1ull)); dsyy = (double)(boxQ >> kSatSqShift16);
            }
            const double num = dn * (double)sxy[i] - dsx * dsy;
            const double P = va * (dn * dsyy - dsy * dsy);
            bool redo;
            float q = (float)mx::ncc_quot_fast(num, P, redo);
            if (redo) q = mx::ncc_quot_exact(num, mx::ncc_den_exact(P));
            val[y * VP + x] = q;
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

template <class Clean, class Dirty>
static hipError_t launch_pair(const MatchU8Args &a, hipStream_t stream)
{
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    hipLaunchKernelGGL(match_ncc_full_u16<Clean>, dim3(nb), dim3(Clean::NT), 0, stream, a);
    hipLaunchKernelGGL(match_ncc_full_u16<Dirty>, dim3(nb), dim3(Dirty::NT), 0, stream, a);
    return hipGetLastError();
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

}  // namespace fu16

hipError_t launch_match_full_u16(MatchU8Args a, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || !a.sat0 || !a.sat1 || !a.satz0 || !a.satz1 || a.full_R < 1 || a.full_R > 15 || (a.Wp & 3)) return hipErrorInvalidValue;
    if (a.full_cand && (a.full_peak || a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks)) return hipErrorInvalidValue;
    if (a.full_surf && a.full_peak) return hipErrorInvalidValue;
    switch (a.ocw) {
    case 7: return fu16::launch_ocw<7>(a, stream);
    case 15: return fu16::launch_ocw<15>(a, stream);
    case 16: return fu16::launch_ocw<16>(a, stream);
    case 30: return fu16::launch_ocw<30>(a, stream);
    case 32: return fu16::launch_ocw<32>(a, stream);
    case 40: return fu16::launch_ocw<40>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mimc3
