// stack_acc.h -- the accumulating (ACC) output form of the four run-time-ocw matrix-core searches (match_full_chip_u8 / _u16,
// match_wide_u8 / _u16 kernels; mimc3_stack_add_fused): a point's finished NCC surface goes from LDS straight into the stack, where the
// SURF form would store it for stack_add_kernel (stack_kernel.hip) to read back.  Every point is finished by exactly one workgroup -- the
// clean form, or the masked form in flag mode behind it -- so one lane owns a cell of the stack for the whole layer: plain
// read-modify-writes, no atomics, no layer scratch.  The state afterwards is stack_add_kernel's over the SURF form's surfaces and records:
// the same f64 additions per cell (a cell takes one addition per layer, so their order within a layer is immaterial), the same u16 wrap
// of cnt and lay.  A SCALED layer (mimc3_stack_add_scaled_fused) goes the same way: stack_acc_scaled resamples the surface from LDS onto the
// stack's cells as stack_add_scaled_kernel does from the layer scratch, with that kernel's stack_scaled_axis, which lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"

namespace mimc3 {
namespace mx {

// lay[pt] of a point that is not refused: what stack_count_layer makes of a record whose status is not -3 (one lane per point calls this)
__device__ __forceinline__ void stack_acc_count(const MatchU8Args &p, int gidx)
{
    uint16_t *__restrict__ lay = p.stk_lay;
    lay[gidx] = (uint16_t)(lay[gidx] + 1);
}

// A point that leaves before its surface exists (the kernels' no_record): no cell; the layer counts unless the status is -3 -- the NaN
// record of a chip or box out of bounds counts, as it does from the record
__device__ __forceinline__ void stack_acc_none(const MatchU8Args &p, int gidx, int tid, float status)
{
    if (tid == 0 && status != -3.0f) stack_acc_count(p, gidx);
}

// The whole workgroup (NT threads), after the barrier that completes val ([S][VP] floats in LDS, cell (x, y) at val[y * VP + x]): the
// cells in the stack's k order, k = x S + y -- the LDS reads at stride VP of the SURF form's store, global read-modify-writes of
// consecutive f64 / u16 over the lanes.  A finite cell adds itself, 1 to cnt and 1.0 to wsum (a weighted stack);
// NaN and +-Inf add nothing
template <int NT, int VP>
__device__ __forceinline__ void stack_acc(const MatchU8Args &p, const float *val, int gidx, int S, int tid)
{
    const int NC = S * S;
    const size_t base = (size_t)gidx * (size_t)NC;
    double *__restrict__ sum = p.stk_sum + base;
    uint16_t *__restrict__ cnt = p.stk_cnt + base;
    double *__restrict__ wsum = p.stk_wsum ? p.stk_wsum + base : nullptr;
    for (int k = tid; k < NC; k += NT) {
        const int x = k / S, y = k - S * x;
        const float v = val[y * VP + x];
        if (__builtin_isfinite(v)) {
            sum[k] += (double)v;
            cnt[k] = (uint16_t)(cnt[k] + 1);
            if (wsum) wsum[k] += 1.0;
        }
    }
    if (tid == 0) stack_acc_count(p, gidx);
}

}  // namespace mx

// ---- a scaled and weighted layer (the definition is in include/mimc3_hip.h) ----
// One axis of a stack cell at displacement d from the stack's shift: the fraction a and the first tap j of the layer's surface (radius
// Rl, searched around lshift).  Every f64 operation is the definition's, in its order (-ffp-contract=off: nothing fuses).  p is s d give
// or take 1/2 and an ulp, so |p| < 64 x 47 + 1 and (int)f is exact.  Shared by stack_add_scaled_kernel (stack_kernel.hip) and
// stack_acc_scaled below.
__device__ __forceinline__ void stack_scaled_axis(double s, int32_t shift, int d, int32_t lshift, int Rl, double &a, int &j)
{
    const double p = s * (double)((int64_t)shift + d) - (double)lshift;
    const double f = __builtin_floor(p);
    a = p - f;
    j = (int)f + Rl;
}

namespace mx {

// The scaled accumulating form (mimc3_stack_add_scaled_fused; p.stk_shift set): the whole workgroup, after the barrier that completes val
// -- the LAYER's surface, Sl x Sl cells searched around p.full_shift (the layer shift), layer cell (ju, jv) at val[jv * VP + ju].  The
// STACK's S^2 cells (S = 2 p.stk_R + 1, independent of Sl) are walked in its k order, k = x S + y, and each does exactly what
// stack_add_scaled_kernel does: both axes by stack_scaled_axis, a tap of weight zero not read, every tap that is read inside the layer,
// the f64 bilinear value in the written order, sum += w value, cnt += 1, wsum += w (a weighted stack).  One lane owns a stack cell for
// the whole layer: plain read-modify-writes of consecutive f64 / u16 over the lanes, no atomics, no layer scratch, no LDS beyond val
template <int NT, int VP>
__device__ __forceinline__ void stack_acc_scaled(const MatchU8Args &p, const float *val, int gidx, int Sl, int tid)
{
    const int R = p.stk_R, S = 2 * R + 1, NC = S * S, Rl = Sl >> 1;
    const double s = p.stk_scale, w = p.stk_weight;
    const int32_t shu = p.stk_shift[2 * (size_t)gidx], shv = p.stk_shift[2 * (size_t)gidx + 1];
    const int32_t lu = p.full_shift ? p.full_shift[2 * (size_t)gidx] : 0, lv = p.full_shift ? p.full_shift[2 * (size_t)gidx + 1] : 0;
    const size_t base = (size_t)gidx * (size_t)NC;
    double *__restrict__ sum = p.stk_sum + base;
    uint16_t *__restrict__ cnt = p.stk_cnt + base;
    double *__restrict__ wsum = p.stk_wsum ? p.stk_wsum + base : nullptr;
    for (int k = tid; k < NC; k += NT) {
        const int x = k / S, y = k - S * x;                      // su = x - R, sv = y - R
        double au, av;
        int ju, jv;
        stack_scaled_axis(s, shu, x - R, lu, Rl, au, ju);
        stack_scaled_axis(s, shv, y - R, lv, Rl, av, jv);
        const bool two_u = au != 0.0, two_v = av != 0.0;          // a tap of weight zero is not read: it may be NaN or lie outside
        if (ju < 0 || jv < 0 || ju + (two_u ? 1 : 0) >= Sl || jv + (two_v ? 1 : 0) >= Sl) continue;
        const float *l0 = val + jv * VP + ju;                    // (ju, jv); (ju, jv + 1) at l0[VP], (ju + 1, jv) at l0[1]
        double value = two_v ? (1.0 - av) * (double)l0[0] + av * (double)l0[VP] : (double)l0[0];
        if (two_u) {
            const float *l1 = l0 + 1;
            const double r1 = two_v ? (1.0 - av) * (double)l1[0] + av * (double)l1[VP] : (double)l1[0];
            value = (1.0 - au) * value + au * r1;
        }
        if (!__builtin_isfinite(value)) continue;
        sum[k] += w * value;
        cnt[k] = (uint16_t)(cnt[k] + 1);
        if (wsum) wsum[k] += w;
    }
    if (tid == 0) stack_acc_count(p, gidx);
}

// the launchers' check of a scaled launch's own arguments (the stack's radius, the scale and the weight: the ranges of the definition)
inline bool stack_acc_scaled_ok(const MatchU8Args &a)
{
    return a.stk_R >= 1 && a.stk_R <= kStackAccMaxRadius && a.stk_scale >= 1.0 / 64 && a.stk_scale <= 64.0 && a.stk_weight > 0.0 &&
           __builtin_isfinite(a.stk_weight);
}

// what the accumulating forms call in the SURF store's place: the scaled form where the launch carries the stack's shift (uniform over
// the launch), else the unscaled one
template <int NT, int VP>
__device__ __forceinline__ void stack_acc_any(const MatchU8Args &p, const float *val, int gidx, int S, int tid)
{
    if (p.stk_shift) stack_acc_scaled<NT, VP>(p, val, gidx, S, tid);
    else stack_acc<NT, VP>(p, val, gidx, S, tid);
}

}  // namespace mx
}  // namespace mimc3
