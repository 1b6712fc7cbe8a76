// match_full_tail.h -- what every front of the exhaustive search shares (internal): the NCC finish of one cell from its exact sums, and
// the tail over the finished f32 surface -- the record (first-wins arg-max, border and validity rules, the 3x3 fit, SNR, Hessian) and
// the candidates (the best local maxima).  Included by match_mx_kernel.hip (8-bit pairs, matrix cores) and match_full_u16_kernel.hip
// (scaled-integer pairs, u16 planes): one text, so the record code of the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"

namespace mimc3 {

namespace mx {

// first-wins arg-max over the 16 lanes of a DPP row (lexicographic max on (value, -index)); VALU only
__device__ __forceinline__ void argmax_row16(float &v, int &i)
{
#define MIMC3_MX_ARGMAX_STEP(ctrl)                                                                        \
    {                                                                                                     \
        const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, true)); \
        const int oi = __builtin_amdgcn_update_dpp(0, i, ctrl, 0xF, 0xF, true);                           \
        const bool t = (ov > v) || (ov == v && oi < i);                                                   \
        v = t ? ov : v; i = t ? oi : i;                                                                   \
    }
    MIMC3_MX_ARGMAX_STEP(0xB1) MIMC3_MX_ARGMAX_STEP(0x4E) MIMC3_MX_ARGMAX_STEP(0x141) MIMC3_MX_ARGMAX_STEP(0x140)
#undef MIMC3_MX_ARGMAX_STEP
}

// ---- NCC of one cell (:734) from its exact sums: the f64 formula rounded to f32 -------------------------------------------------
//   reference:  (float)( num / sqrt(P) ),  num = n sxy - sx sy  and  va = n sxx - sx^2,  vb = n syy - sy^2  exact integers in f64,
//               P = va * vb rounded once, sqrt and the division correctly rounded: the f64 quotient Qd is within 2^-51 of num / sqrt(P).
//   fast:       r = v_rsq_f64(P) refined by one Newton step (relative error 2^-47.8 measured, tools/probes/mx_finish.hip; the
//               instruction alone 2^-24.2), Q' = num * r'.  Q' and Qd round to the SAME f32 unless an f32 rounding boundary lies
//               between them: a cell whose Q' is within 2^13 f64 ulps (2^-40 relative) of a boundary, or whose P is not positive (the
//               reference's inf / NaN cases), reports redo and is computed again by ncc_den_exact and ncc_quot_exact.
//               2^-15 of the cells; over 2^34 random cells the farthest one whose two results differed lay 7 ulps from its boundary.
__device__ __forceinline__ double ncc_quot_fast(double num, double P, bool &redo)
{
    const double r = __builtin_amdgcn_rsq(P);
    const double g = P * r;
    const double e2 = __builtin_fma(-r, g, 1.0);
    const double r1 = __builtin_fma(0.5 * r, e2, r);
    const double q = num * r1;
    const uint32_t low = ((uint32_t)__double2loint(q) & 0x1fffffffu) - (0x10000000u - 0x2000u);     // distance to the f32 rounding boundary, + 2^13
    redo = !(P > 0.0) || low <= 0x4000u;
    return q;                           // (the caller rounds it to f32)
}
// the reference's own operations: den = sqrt(P), then the division, both correctly rounded
__device__ __forceinline__ double ncc_den_exact(double P) { return sqrt(P); }
__device__ __forceinline__ float ncc_quot_exact(double num, double den) { return (float)(num / den); }

// ---- full mode (FullCfg) ----------------------------------------------------------------------------------------------
// a record without a fit: the status (-2 no finite cell, -3 invalid, -4 peak on the border) in column 2, NaN elsewhere
__device__ __forceinline__ void full_store(float *o, float status)
{
    const float nanv = __builtin_nanf("");
    o[0] = nanv; o[1] = nanv; o[2] = status;
#pragma unroll
    for (int i = 3; i < 8; i++) o[i] = nanv;
}

// (FullMultiCfg) every candidate slot of a point that has no surface: (NaN, NaN, status)
template <class C>
__device__ __forceinline__ void full_cand_fill(const MatchU8Args &p, int gidx, float status)
{
    if constexpr (C::MULTI) {
        const float nanv = __builtin_nanf("");
        for (int j = 0; j < p.full_npeaks; j++) {
            float *q = p.full_cand + 3 * ((size_t)j * (size_t)p.N + (size_t)gidx);
            q[0] = nanv; q[1] = nanv; q[2] = status;
        }
    }
}

// The tail of the exhaustive search on wave 0, over the f32 surface val[y][x] (tile cell (x, y) = offset (x - R, y - R)):
//   peak   first-wins arg-max over the finite cells in k = (su + R)(2R + 1) + (sv + R) (u outer): lane l scans k = l, l + 64, ...
//          in ascending order (strict >: its first maximum), then the lanes (value, -k) lexicographically (argmax_row16, then
//          across the rows);
//   fit    the reference's 3x3 quadratic (:757-788) value by value, float / double mix as there (match_ncc_dlc_mx's fit), plus
//          the model's value at its extremum (c5 the constant of the same least-squares fit) and its Hessian 2 c0, c1, 2 c2;
//   snr    ncc_peak^2 / mean(NCC^2) over the finite cells outside the peak's 3x3 block (f64 partial sums per lane, then a tree).
template <class C>
__device__ __forceinline__ void full_peak_store(const MatchU8Args &p, int gidx, int k)
{
    if constexpr (C::PEAK) p.full_peak[gidx] = k;
}

template <class C>
__device__ __forceinline__ void full_tail(const MatchU8Args &p, const float *val, int gidx, int shu, int shv, int lane)
{
    constexpr int VP = C::VP;
    const int R = p.full_R, S = 2 * R + 1, NC = S * S;
    float *out = p.out + 8 * (size_t)gidx;
    float bv = -__builtin_inff();
    int bk = 0x7fffffff;
    for (int k = lane; k < NC; k += 64) {
        const int x = k / S, y = k - S * x;
        const float v = val[y * VP + x];
        if (__builtin_isfinite(v) && v > bv) { bv = v; bk = k; }
    }
    argmax_row16(bv, bk);
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bk, o, 64);
        if (ov > bv || (ov == bv && oi < bk)) { bv = ov; bk = oi; }
    }
    bv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bv)));
    bk = __builtin_amdgcn_readfirstlane(bk);
    if (bk == 0x7fffffff) { if (lane == 0) { full_store(out, -2.0f); full_peak_store<C>(p, gidx, -1); } return; }
    const int px = bk / S, py = bk - S * px, su = px - R, sv = py - R;
    if (su == -R || su == R || sv == -R || sv == R) { if (lane == 0) { full_store(out, -4.0f); full_peak_store<C>(p, gidx, bk); } return; }
    double s2 = 0.0;
    int cnt = 0;
    for (int k = lane; k < NC; k += 64) {
        const int x = k / S, y = k - S * x;
        const float v = val[y * VP + x];
        const bool near = x - px <= 1 && px - x <= 1 && y - py <= 1 && py - y <= 1;
        if (__builtin_isfinite(v) && !near) { s2 += (double)v * (double)v; cnt++; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { s2 += __shfl_xor(s2, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if (lane != 0) return;
    float n9[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) n9[3 * r + c] = val[(py - 1 + r) * VP + (px - 1 + c)];
    const float e0 = 6 * n9[0] - 12 * n9[1] + 6 * n9[2] + 6 * n9[3] - 12 * n9[4] + 6 * n9[5] + 6 * n9[6] - 12 * n9[7] + 6 * n9[8];
    const float e1 = 9 * n9[0] - 9 * n9[2] - 9 * n9[6] + 9 * n9[8];
    const float e2 = 6 * n9[0] + 6 * n9[1] + 6 * n9[2] - 12 * n9[3] - 12 * n9[4] - 12 * n9[5] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
    const float e3 = -6 * n9[0] + 6 * n9[2] - 6 * n9[3] + 6 * n9[5] - 6 * n9[6] + 6 * n9[8];
    const float e4 = -6 * n9[0] - 6 * n9[1] - 6 * n9[2] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
    const float e5 = -4 * n9[0] + 8 * n9[1] - 4 * n9[2] + 8 * n9[3] + 20 * n9[4] + 8 * n9[5] - 4 * n9[6] + 8 * n9[7] - 4 * n9[8];
    double c0 = e0, c1 = e1, c2 = e2, c3 = e3, c4 = e4, c5 = e5;
    c0 /= 36; c1 /= 36; c2 /= 36; c3 /= 36; c4 /= 36; c5 /= 36;
    const float nu = (float)(-2 * c2 * c3 + c1 * c4), nv = (float)(-2 * c0 * c4 + c1 * c3);
    const double det = 4 * c0 * c2 - c1 * c1;
    float du = (float)((double)nu / det), dv = (float)((double)nv / det);
    du += (float)(su + shu);
    dv += (float)(sv + shv);
    const double xs = (-2 * c2 * c3 + c1 * c4) / det, ys = (-2 * c0 * c4 + c1 * c3) / det;
    const double fit = c0 * xs * xs + c1 * xs * ys + c2 * ys * ys + c3 * xs + c4 * ys + c5;
    const double snr = cnt > 0 ? ((double)bv * (double)bv) / (s2 / (double)cnt) : (double)__builtin_nan("");
    out[0] = du; out[1] = dv; out[2] = bv; out[3] = (float)fit; out[4] = (float)snr;
    out[5] = (float)(2 * c0); out[6] = (float)c1; out[7] = (float)(2 * c2);
    full_peak_store<C>(p, gidx, bk);
}

// The candidates of the exhaustive search (FullMultiCfg), on wave 0 behind full_tail, which has written the record -- also where it
// has no fit (-2: there is no local maximum either; -4: the interior ones are the candidates):
//   scan     lane l tests its cells k = l, l + 64, ... for the local-maximum rule: interior (|su|, |sv| < R), finite, and against each of
//            the 8 neighbours t: t not finite, NCC(s) > NCC(t), or equal with k(s) < k(t) (a plateau yields its lowest k alone).  One
//            bit per cell of the lane: at most 16;
//   select   full_npeaks rounds of the wave arg-max (value descending, k ascending): a lane offers its best local maximum strictly
//            behind the previous round's pick in that order -- no list, no atomics; round j's pick stays with lane j;
//   fit      lanes 0 .. full_npeaks - 1 fit one candidate each: the reference's 3x3 quadratic, the expressions of full_tail.
// Slots beyond the last local maximum: (NaN, NaN, -2).
template <class C>
__device__ __forceinline__ void full_tail_multi(const MatchU8Args &p, const float *val, int gidx, int shu, int shv, int lane)
{
    constexpr int VP = C::VP;
    constexpr int kNone = 0x7fffffff;
    const int R = p.full_R, S = 2 * R + 1, NC = S * S, npk = p.full_npeaks;
    const float invS = 1.0f / (float)S;
    // k / S for k < 1024, S <= 31: (k + 1/2) / S lies at least 1 / 62 from an integer, the f32 product within 2^-16 of it
    auto col_of = [&](int k) __attribute__((always_inline)) -> int { return (int)(((float)k + 0.5f) * invS); };
    uint32_t lm = 0u;
    {
        int j = 0;
        for (int k = lane; k < NC; k += 64, j++) {
            const int x = col_of(k), y = k - S * x;
            const bool interior = x >= 1 && x <= S - 2 && y >= 1 && y <= S - 2;
            const float *c = val + (interior ? y : 1) * VP + (interior ? x : 1);      // (a border cell reads a harmless block)
            const float v = c[0];
            bool ok = interior && __builtin_isfinite(v);
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
                    if (dx == 0 && dy == 0) continue;
                    const float t = c[dy * VP + dx];
                    const bool later = dx > 0 || (dx == 0 && dy > 0);                    // k(t) > k(s)
                    ok = ok && (!__builtin_isfinite(t) || v > t || (later && v == t));
                }
            lm |= (ok ? 1u : 0u) << j;
        }
    }
    float pv = __builtin_inff(), myv = 0.0f;
    int pk = -1, myk = kNone;
    for (int r = 0; r < npk; r++) {
        float bv = -__builtin_inff();
        int bk = kNone;
        for (uint32_t m = lm; m != 0u; m &= m - 1u) {        // ascending k: strict > keeps the lane's first
            const int k = lane + 64 * (__builtin_ffs((int)m) - 1);
            const int x = col_of(k), y = k - S * x;
            const float v = val[y * VP + x];
            const bool behind = v < pv || (v == pv && k > pk);
            if (behind && v > bv) { bv = v; bk = k; }
        }
        argmax_row16(bv, bk);
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bk, o, 64);
            if (ov > bv || (ov == bv && oi < bk)) { bv = ov; bk = oi; }
        }
        bv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bv)));
        bk = __builtin_amdgcn_readfirstlane(bk);
        if (bk == kNone) break;
        if (lane == r) { myv = bv; myk = bk; }
        pv = bv; pk = bk;
    }
    if (lane >= npk) return;
    float *q = p.full_cand + 3 * ((size_t)lane * (size_t)p.N + (size_t)gidx);
    if (myk == kNone) { const float nanv = __builtin_nanf(""); q[0] = nanv; q[1] = nanv; q[2] = -2.0f; return; }
    const int px = col_of(myk), py = myk - S * px, su = px - R, sv = py - R;
    float n9[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) n9[3 * r + c] = val[(py - 1 + r) * VP + (px - 1 + c)];
    const float e0 = 6 * n9[0] - 12 * n9[1] + 6 * n9[2] + 6 * n9[3] - 12 * n9[4] + 6 * n9[5] + 6 * n9[6] - 12 * n9[7] + 6 * n9[8];
    const float e1 = 9 * n9[0] - 9 * n9[2] - 9 * n9[6] + 9 * n9[8];
    const float e2 = 6 * n9[0] + 6 * n9[1] + 6 * n9[2] - 12 * n9[3] - 12 * n9[4] - 12 * n9[5] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
    const float e3 = -6 * n9[0] + 6 * n9[2] - 6 * n9[3] + 6 * n9[5] - 6 * n9[6] + 6 * n9[8];
    const float e4 = -6 * n9[0] - 6 * n9[1] - 6 * n9[2] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
    double c0 = e0, c1 = e1, c2 = e2, c3 = e3, c4 = e4;
    c0 /= 36; c1 /= 36; c2 /= 36; c3 /= 36; c4 /= 36;
    const float nu = (float)(-2 * c2 * c3 + c1 * c4), nv = (float)(-2 * c0 * c4 + c1 * c3);
    const double det = 4 * c0 * c2 - c1 * c1;
    float du = (float)((double)nu / det), dv = (float)((double)nv / det);
    du += (float)(su + shu);
    dv += (float)(sv + shv);
    q[0] = du; q[1] = dv; q[2] = myv;
}

}  // namespace mx

}  // namespace mimc3
