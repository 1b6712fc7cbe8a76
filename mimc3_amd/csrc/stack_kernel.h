// stack_kernel.h -- the two kernels of NCC stacking (mimc3_stack_*, capi.cpp; the contract is in include/mimc3_hip.h): the accumulation
// of one layer of surfaces into the stack, and the tail of the exhaustive search (match_full_tail.h) over the stack's mean surface.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mimc3 {

constexpr int kStackChunk = 65536;      // MIMC3_STACK_CHUNK: the points of one launch of the accumulation

// One layer over n <= kStackChunk points, NC = (2R+1)^2 cells each, in the surface's k order: for every cell of surf [n][NC] that is
// finite, sum += (double)v and cnt += 1 (NaN and +-Inf add nothing); for every point that is not refused, lay += 1.  A point is refused
// when rec (the search's records [n][8], or null) has -3 in column 2, or when refused ([n], or null) is not 0; with both null no point is.
// sum, cnt and lay point at the first of the n points.  One lane owns a cell: plain read-modify-writes, no atomics.  surf needs no
// alignment beyond a float's; cells are read four at a time where surf, sum and cnt are 16-, 16- and 8-byte aligned.
hipError_t launch_stack_add(const float *surf, const float *rec, const uint8_t *refused, int n, int NC, double *sum, uint16_t *cnt,
                            uint16_t *lay, hipStream_t s);

// The result over all N points: mean[k] = (float)(sum[k] / (double)cnt[k]) where cnt[k] >= min_count (>= 1), NaN elsewhere; a point with
// lay == 0 gets status -3 in its record and every candidate slot, any other the tail of match_full_tail.h over mean with shift [N][2]
// (or null).  out [N][8]; cand [npeaks][N][3], null iff npeaks == 0; surf [N][NC] (mean) and count [N] (lay) optional.  Reads the stack
// and leaves it unchanged.
hipError_t launch_stack_tail(const double *sum, const uint16_t *cnt, const uint16_t *lay, const int32_t *shift, int N, int R, int npeaks,
                             int min_count, float *out, float *cand, float *surf, uint16_t *count, hipStream_t s);

}  // namespace mimc3
