// stack_kernel.h -- the kernels of NCC stacking (mimc3_stack_*, capi.cpp; the contract is in include/mimc3_hip.h): the accumulation
// of one layer of surfaces into the stack, the same for a layer of another time baseline (scaled, weighted), and the tail of the
// exhaustive search (match_full_tail.h) over the stack's mean surface.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mimc3 {

constexpr int kStackChunk = 65536;      // MIMC3_STACK_CHUNK: the points of one launch of the accumulation (R <= 15)
constexpr int kStackMaxRadius = 47;     // the largest mimc3_wide_max_radius: a 95 x 95 surface
constexpr int64_t kStackChunkCells = (int64_t)kStackChunk * 961;      // the cells of one launch: what a chunk holds at R 15

// mimc3_stack_chunk: the points of one launch of the accumulation at radius R -- kStackChunk up to R 15, beyond it as many as keep the
// launch's cells at kStackChunkCells (the layer scratch stays at 252 MB, n NC below 2^26 for stack_add_kernel's 32-bit indices);
// 0 for an R that no stack takes
constexpr int stack_chunk(int R)
{
    return R < 1 || R > kStackMaxRadius ? 0 : R <= 15 ? kStackChunk : (int)(kStackChunkCells / ((2 * R + 1) * (2 * R + 1)));
}
static_assert(stack_chunk(16) == 57832 && stack_chunk(47) == 6978, "mimc3_hip.h quotes these");

// One layer over n <= stack_chunk(R) points, NC = (2R+1)^2 <= 9,025 cells each, in the surface's k order: for every cell of surf [n][NC] that is
// finite, sum += (double)v and cnt += 1 (NaN and +-Inf add nothing); for every point that is not refused, lay += 1.  A point is refused
// when rec (the search's records [n][8], or null) has -3 in column 2, or when refused ([n], or null) is not 0; with both null no point is.
// sum, cnt and lay point at the first of the n points.  One lane owns a cell: plain read-modify-writes, no atomics.  surf needs no
// alignment beyond a float's; cells are read four at a time where surf, sum and cnt are 16-, 16- and 8-byte aligned.  wsum (a weighted
// stack's third plane, or null) gets += 1.0 wherever cnt gets += 1.
hipError_t launch_stack_add(const float *surf, const float *rec, const uint8_t *refused, int n, int NC, double *sum, uint16_t *cnt,
                            uint16_t *lay, double *wsum, hipStream_t s);

// One scaled layer over n points (n (2R+1)^2 and n (2Rl+1)^2 both <= kStackChunkCells): surf [n][(2Rl+1)^2] was searched around lshift
// [n][2] = rint(scale shift); every stack cell takes the bilinear value of its point's surface at scale x (shift + cell) - lshift by the
// definition of mimc3_hip.h -- sum += weight * value, cnt += 1, wsum += weight (wsum null on a stack that is not weighted) where every
// tap that is read lies inside the surface and the value is finite; lay as launch_stack_add.  1/64 <= scale <= 64, weight > 0 and
// finite; R and Rl in 1..kStackMaxRadius, independently.  One workgroup per point (one wave where R, Rl <= 15, four beyond), the
// surface in dynamic LDS (36,100 bytes at Rl 47).
hipError_t launch_stack_add_scaled(const float *surf, const float *rec, const uint8_t *refused, const int32_t *shift, const int32_t *lshift,
                                   int n, int R, int Rl, double scale, double weight, double *sum, uint16_t *cnt, double *wsum,
                                   uint16_t *lay, hipStream_t s);

// lshift [N][2] = (int32)rint(scale (double)shift [N][2]): one f64 product, rounded half to even (the caller has checked its range)
hipError_t launch_stack_layer_shift(const int32_t *shift, int N, double scale, int32_t *lshift, hipStream_t s);

// wsum[i] = (double)cnt[i] over the stack's cells: what a stack's first weighted add starts from
hipError_t launch_stack_wsum_init(const uint16_t *cnt, size_t cells, double *wsum, hipStream_t s);

// The result over all N points: mean[k] = (float)(sum[k] / (double)cnt[k]) -- with wsum (or null), (float)(sum[k] / wsum[k]) -- where
// cnt[k] >= min_count (>= 1), NaN elsewhere; a point with
// lay == 0 gets status -3 in its record and every candidate slot, any other the tail of match_full_tail.h over mean with shift [N][2]
// (or null).  R <= 15: one wave per point; 16 <= R <= kStackMaxRadius: one workgroup per point, the candidates by match_wide_tail.h.  out [N][8]; cand [npeaks][N][3], null iff npeaks == 0; surf [N][NC] (mean) and count [N] (lay) optional.  Reads the stack
// and leaves it unchanged.
hipError_t launch_stack_tail(const double *sum, const uint16_t *cnt, const uint16_t *lay, const double *wsum, const int32_t *shift, int N,
                             int R, int npeaks, int min_count, float *out, float *cand, float *surf, uint16_t *count, hipStream_t s);

}  // namespace mimc3
