// match_wide_tail.h -- the candidate tail of the exhaustive search for surfaces of any size (internal; match_wide_kernel.hip).
//
// match_full_tail.h's full_tail_multi keeps one bit per cell in a 32-bit mask per lane and divides by S with an f32 product argued for
// k < 1024: both stop at a 31 x 31 surface.  This is the same rule and the same ranked selection, statement by statement, for up to
// 95 x 95 cells (any S with S^2 <= 64 * 32 * kWideLmWords):
//   rule     s is a local maximum when it is interior (|su|, |sv| < R), finite, and for each of its 8 neighbours t: t not finite,
//            NCC(s) > NCC(t), or equal with k(s) < k(t) (a plateau yields its lowest k alone);
//   plane    wide_lm_plane: ALL waves of the workgroup apply the rule once, into a bit plane in LDS -- lane l of the tail owns the cells
//            k = l + 64 j; bit (j & 31) of word bits[(j >> 5) * 64 + l].  Thread (wave w, lane l) builds the words w, w + 4, ... of lane l
//            whole, in registers: no atomics.  (x, y) of a cell is walked, k + 64 = (x + 64 / S, y + 64 % S) with one carry;
//   select   wave 0, full_npeaks rounds of the wave arg-max (value descending, k ascending): a lane offers its best local maximum
//            strictly behind the previous round's pick; round j's pick stays with lane j.  A lane holds its words in registers and
//            visits set bits only; a set bit's (x, y) comes from an integer division;
//   fit      lanes 0 .. full_npeaks - 1 fit one candidate each: the reference's 3x3 quadratic, the expressions of full_tail.
// Slots beyond the last local maximum: (NaN, NaN, -2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "match_full_tail.h"

namespace mimc3 {

namespace mx {

constexpr int kWideLmWords = 5;                                 // 64 lanes x 5 words x 32 bits = 10,240 cells >= 95 x 95
constexpr int kWideLmBytes = 64 * kWideLmWords * 4;

// every thread of the workgroup (NT a multiple of 64); val is complete and bits is not read before the next barrier
template <class C>
__device__ __forceinline__ void wide_lm_plane(const MatchU8Args &p, const float *val, uint32_t *bits, int tid)
{
    constexpr int VP = C::VP, NW = C::NT / 64;
    const int R = p.full_R, S = 2 * R + 1, NC = S * S;
    const int lane = tid & 63, wave = tid >> 6;
    const int q64 = 64 / S, r64 = 64 - S * q64;
    for (int w = wave; w < kWideLmWords; w += NW) {
        const int k0 = lane + 64 * 32 * w;
        uint32_t m = 0u;
        if (k0 < NC) {
            int x = k0 / S, y = k0 - S * x, k = k0;
            for (int b = 0; b < 32 && k < NC; b++, k += 64) {
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
                m |= (ok ? 1u : 0u) << b;
                x += q64; y += r64;
                if (y >= S) { y -= S; x++; }
            }
        }
        bits[w * 64 + lane] = m;
    }
}

// wave 0, behind full_tail (which has written the record) and a barrier behind wide_lm_plane
template <class C>
__device__ __forceinline__ void wide_tail_multi(const MatchU8Args &p, const float *val, const uint32_t *bits, int gidx, int shu, int shv,
                                                int lane)
{
    constexpr int VP = C::VP;
    constexpr int kNone = 0x7fffffff;
    const int R = p.full_R, S = 2 * R + 1, npk = p.full_npeaks;
    uint32_t lm[kWideLmWords];
#pragma unroll
    for (int w = 0; w < kWideLmWords; w++) lm[w] = bits[w * 64 + lane];
    float pv = __builtin_inff(), myv = 0.0f;
    int pk = -1, myk = kNone;
    for (int r = 0; r < npk; r++) {
        float bv = -__builtin_inff();
        int bk = kNone;
#pragma unroll
        for (int w = 0; w < kWideLmWords; w++)
            for (uint32_t m = lm[w]; m != 0u; m &= m - 1u) {         // ascending k: strict > keeps the lane's first
                const int k = lane + 64 * (32 * w + __builtin_ffs((int)m) - 1);
                const int x = k / S, y = k - S * x;
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
    const int px = myk / S, py = myk - S * px, su = px - R, sv = py - R;
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
