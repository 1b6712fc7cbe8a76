// stack_acc.h -- the accumulating (ACC) output form of the four run-time-ocw matrix-core searches (match_full_chip_u8 / _u16,
// match_wide_u8 / _u16 kernels; mimc3_stack_add_fused): a point's finished NCC surface goes from LDS straight into the stack, where the
// SURF form would store it for stack_add_kernel (stack_kernel.hip) to read back.  Every point is finished by exactly one workgroup -- the
// clean form, or the masked form in flag mode behind it -- so one lane owns a cell of the stack for the whole layer: plain
// read-modify-writes, no atomics, no layer scratch.  The state afterwards is stack_add_kernel's over the SURF form's surfaces and records:
// the same f64 additions per cell (a cell takes one addition per layer, so their order within a layer is immaterial), the same u16 wrap
// of cnt and lay.
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
}  // namespace mimc3
