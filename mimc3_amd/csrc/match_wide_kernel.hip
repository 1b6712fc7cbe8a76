// match_wide_kernel.hip -- exhaustive-search NCC offsets beyond +-15 px for gfx950 (mimc3_match_ncc_wide): one exact pass at full
// resolution over a search range of up to +-47 px, with the record, the candidates and the surfaces of mimc3_match_ncc_full_any (mode 1).
//
// The definition is match_full_f32g_kernel.hip's, word for word: the zero-bordered f32 planes of any pair, the reference's two null
// rules (validity counts p < MIN_DN, a NaN is not counted; inclusion a >= MIN_DN && b >= MIN_DN, a NaN is excluded), f32 products widened
// to f64, ADDITIONS ONLY, the finish with the reference's f64 operations.  So is the structure: one workgroup of four wave64 = one grid
// point; box and chip in LDS as f32, an excluded pixel staged as 0; the counts under both rules and the chip's sx, sxx taken while
// staging; a clean and a dirty body chosen per workgroup; a task = one surface row y and four neighbouring cells x0 .. x0 + 3, and the
// clean body's box sums shared among the four (one core accumulator and six edge sums per row).
//
// What a search range of up to 95 x 95 cells changes:
//   tasks are walked   S ceil(S / 4) tasks (2,280 at S = 95) for 256 threads: a thread takes the tasks tid, tid + 256, ... and sums ALL
//                      chip rows of a task itself, in row order -- no slices, no shuffle tree -- finishes its four cells and writes them.
//                      The order of every sum is therefore a function of ocw alone.
//   LDS by R           box rows of PB(R) floats: the pixels a row's tasks read (CWP + 4 ceil(S / 4)), padded to an odd number of 16-byte
//                      slots; behind the box the chip, and behind the chip the surface with bytes of its own (pitch VP = 96 words,
//                      S rows), because the chip is read until the last task.  wide_max_radius(ocw) is the largest R whose layout,
//                      static slots included, fits gfx950's 160 KB -- from the same constexpr the launch uses.
//   tails              the record is mx::full_tail, unedited (it depends on the run-time R and the pitch alone); the candidates are
//                      match_wide_tail.h's: all four waves mark the local maxima in a bit plane (in the box's bytes, dead by then), wave 0
//                      selects and fits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "match_full_tail.h"
#include "match_wide_tail.h"

namespace mimc3 {

namespace wide {

struct Slots {                          // the static LDS of the kernel: the per-wave partial counts and sums of the staging
    double d[4][2];
    int i[4][4];
};

template <int OCW_, bool MULTI_>
struct Cfg {
    static constexpr int OCW = OCW_, CW = 2 * OCW_ + 1, NPX = CW * CW;
    static constexpr bool PEAK = false, MULTI = MULTI_;         // (what match_full_tail.h asks of a configuration)
    static constexpr int VP = 96;                               // pitch (words) of the NCC surface: S <= 95
    static constexpr int NT = 256;
    static constexpr int RCAP = 47;
    static constexpr int CWP = (CW + 3) & ~3;                   // chip row pitch (pixels): whole 4-pixel chunks, zeros behind the chip
    static constexpr int NCH = CWP / 4;
    static constexpr int CHIPB = (CW * CWP * 4 + 15) & ~15;
    static constexpr int ngx(int R) { return (2 * R + 1 + 3) >> 2; }                // tasks per surface row
    static constexpr int bw(int R) { return CWP + 4 * ngx(R); }                     // box pixels a row's tasks read: x0 + the chunks + the one read ahead
    static constexpr int pb(int R) { return ((bw(R) / 4) & 1) ? bw(R) : bw(R) + 4; }        // box row pitch: an odd number of 16-byte slots
    static constexpr int box_bytes(int R) { return (CW + 2 * R) * pb(R) * 4; }
    static constexpr int surf_bytes(int R) { return ((2 * R + 1) * VP * 4 + 15) & ~15; }
    static constexpr int lds_bytes(int R) { return box_bytes(R) + CHIPB + surf_bytes(R); }
    static constexpr bool fits(int R) { return lds_bytes(R) + (int)sizeof(Slots) <= 160 * 1024; }
    // the largest R <= RCAP such that every radius up to it fits a CU's LDS (the pitch's parity rule makes the bytes not quite monotonic)
    static constexpr int max_radius() { int R = 0; while (R < RCAP && fits(R + 1)) R++; return R; }
    static_assert(CWP - CW == 1 || CWP - CW == 3, "the edge pixels CW .. CW + 2 sit in the last chunk and the one read ahead");
    static_assert(2 * RCAP + 1 < VP, "the surface pitch");
    static_assert((2 * RCAP + 1) * (2 * RCAP + 1) <= 64 * 32 * mx::kWideLmWords, "the bit plane of the candidate tail");
    static_assert(box_bytes(1) >= mx::kWideLmBytes, "the bit plane takes the box's place");
};

constexpr double kMinDn = 1e-10;        // MIN_DN (MIMC_module.c:21), compared in double as there

template <class C>
__global__ __launch_bounds__(C::NT) void match_ncc_wide(MatchU8Args p, float *surf)
{
    constexpr int OCW = C::OCW, CW = C::CW, NPX = C::NPX, VP = C::VP, NT = C::NT, CWP = C::CWP, NCH = C::NCH;
    static_assert(C::max_radius() >= 16, "the kernel has a range of its own at every chip size");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ Slots red;
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
    const int PB = C::pb(R);
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
    float *CHIP = reinterpret_cast<float *>(smem + (size_t)D2 * PB * 4);
    float *val = reinterpret_cast<float *>(smem + (size_t)D2 * PB * 4 + C::CHIPB);

    // ---- stage the box and the chip (a wave takes whole rows): count under the two rules, canonical null for every excluded pixel; the
    //      chip's sx and sxx ----
    int c_lt = 0, c_ex = 0, b_lt = 0, b_ex = 0;
    double csx = 0.0, csxx = 0.0;
    {
        const float *g0 = win_pl + (size_t)wv0 * Wp + wu0;
        for (int y = wave; y < D2; y += 4)
            for (int j = lane; j < PB; j += 64) {
                float v = 0.0f;
                if (j < D2) {
                    v = g0[(size_t)y * Wp + j];
                    const double d = (double)v;
                    b_lt += (d < kMinDn) ? 1 : 0;
                    if (!(d >= kMinDn)) { b_ex++; v = 0.0f; }
                }
                BOX[y * PB + j] = v;
            }
        const float *c0 = chip_pl + (size_t)cv0 * Wp + cu0;
        for (int y = wave; y < CW; y += 4)
            for (int j = lane; j < CWP; j += 64) {
                float v = 0.0f;
                if (j < CW) {
                    v = c0[(size_t)y * Wp + j];
                    const double d = (double)v;
                    c_lt += (d < kMinDn) ? 1 : 0;
                    if (!(d >= kMinDn)) { c_ex++; v = 0.0f; }
                    else { csx += d; csxx += (double)(v * v); }
                }
                CHIP[y * CWP + j] = v;
            }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        c_lt += __shfl_xor(c_lt, o, 64); c_ex += __shfl_xor(c_ex, o, 64);
        b_lt += __shfl_xor(b_lt, o, 64); b_ex += __shfl_xor(b_ex, o, 64);
        csx += __shfl_xor(csx, o, 64); csxx += __shfl_xor(csxx, o, 64);
    }
    if (lane == 0) {
        red.i[wave][0] = c_lt; red.i[wave][1] = c_ex; red.i[wave][2] = b_lt; red.i[wave][3] = b_ex;
        red.d[wave][0] = csx; red.d[wave][1] = csxx;
    }
    __syncthreads();
    c_lt = red.i[0][0] + red.i[1][0] + red.i[2][0] + red.i[3][0];
    c_ex = red.i[0][1] + red.i[1][1] + red.i[2][1] + red.i[3][1];
    b_lt = red.i[0][2] + red.i[1][2] + red.i[2][2] + red.i[3][2];
    b_ex = red.i[0][3] + red.i[1][3] + red.i[2][3] + red.i[3][3];
    csx = (red.d[0][0] + red.d[1][0]) + (red.d[2][0] + red.d[3][0]);
    csxx = (red.d[0][1] + red.d[1][1]) + (red.d[2][1] + red.d[3][1]);
    {
        const float max_ratio = 0.8f;
        const float rc = (float)c_lt / (float)NPX;
        const float rw = (float)b_lt / (float)(D2 * D2);
        if (rc > max_ratio || rw > max_ratio) { no_record(-3.0f); return; }
    }
    const bool dirty = (c_ex | b_ex) != 0;                  // workgroup-uniform

    // ---- the tasks: surface row y, cells x0 .. x0 + 3, every chip row; a thread walks tid, tid + NT, ... ---------------------------
    const int NGX = (S + 3) >> 2, ntask = S * NGX;
    for (int task = tid; task < ntask; task += NT) {
        const int y = task / NGX, x0 = 4 * (task - NGX * y);
        double sxy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0}, syy[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
        int cn[4] = {0, 0, 0, 0};
        if (!dirty) {
            double core = 0.0, core2 = 0.0, e[6] = {0, 0, 0, 0, 0, 0}, e2[6] = {0, 0, 0, 0, 0, 0};
            for (int r = 0; r < CW; r++) {
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
            for (int r = 0; r < CW; r++) {
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
        // NCC of this task's cells (:734): the reference's f64 operations one by one; the surface has bytes of its own
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
    __syncthreads();                                        // the surface is complete; box and chip are dead
    if (sf)
        for (int k = tid; k < NC; k += NT) {
            const int x = k / S, yy = k - S * x;
            sf[k] = val[yy * VP + x];
        }
    uint32_t *bits = reinterpret_cast<uint32_t *>(smem);    // (the box's bytes)
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
    if (a.full_R > C::max_radius()) return hipErrorInvalidValue;
    const unsigned nb = (unsigned)((a.N + 7) & ~7);
    const int lds = C::lds_bytes(a.full_R);
    if (lds > 60 * 1024) {              // near or beyond the default limit of LDS, the static slots included (gfx950 has 160 KB per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&match_ncc_wide<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(match_ncc_wide<C>, dim3(nb), dim3(C::NT), lds, stream, a, surf);
    return hipGetLastError();
}

template <int OCW>
static hipError_t launch_ocw(const MatchU8Args &a, float *surf, hipStream_t stream)
{
    if (a.full_cand) return launch_one<Cfg<OCW, true>>(a, surf, stream);
    return launch_one<Cfg<OCW, false>>(a, surf, stream);
}

}  // namespace wide

int wide_max_radius(int ocw)
{
    switch (ocw) {
    case 7: return wide::Cfg<7, false>::max_radius();
    case 15: return wide::Cfg<15, false>::max_radius();
    case 16: return wide::Cfg<16, false>::max_radius();
    case 30: return wide::Cfg<30, false>::max_radius();
    case 32: return wide::Cfg<32, false>::max_radius();
    case 40: return wide::Cfg<40, false>::max_radius();
    default: return 0;
    }
}

int wide_lds_bytes(int ocw, int R)
{
    if (R < 1 || R > wide_max_radius(ocw)) return 0;
    switch (ocw) {
    case 7: return wide::Cfg<7, false>::lds_bytes(R);
    case 15: return wide::Cfg<15, false>::lds_bytes(R);
    case 16: return wide::Cfg<16, false>::lds_bytes(R);
    case 30: return wide::Cfg<30, false>::lds_bytes(R);
    case 32: return wide::Cfg<32, false>::lds_bytes(R);
    case 40: return wide::Cfg<40, false>::lds_bytes(R);
    default: return 0;
    }
}

hipError_t launch_match_wide(MatchU8Args a, float *surf, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.p0 || !a.p1 || a.full_peak || a.full_R < 1 || a.full_R > wide_max_radius(a.ocw)) return hipErrorInvalidValue;
    if (a.full_cand && (a.full_npeaks < 1 || a.full_npeaks > kFullMaxPeaks)) return hipErrorInvalidValue;
    switch (a.ocw) {
    case 7: return wide::launch_ocw<7>(a, surf, stream);
    case 15: return wide::launch_ocw<15>(a, surf, stream);
    case 16: return wide::launch_ocw<16>(a, surf, stream);
    case 30: return wide::launch_ocw<30>(a, surf, stream);
    case 32: return wide::launch_ocw<32>(a, surf, stream);
    case 40: return wide::launch_ocw<40>(a, surf, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mimc3
