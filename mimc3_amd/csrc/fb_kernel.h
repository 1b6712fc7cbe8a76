// fb_kernel.h -- the two elementwise kernels of the forward-backward consistency check (mimc3_match_ncc_full_fb, capi.cpp): the seed of
// the backward search from the forward results, and the composition of the fb rows from the backward records.  The searches themselves
// are mimc3_match_ncc_full_any's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mimc3 {

// why a row of the backward search is not searched (one byte per row; 0 = it is)
constexpr uint8_t kFbSearch = 0, kFbNoFit = 5, kFbLeaves = 6;

// Rows t = plane * N + i, plane 0 = the forward record out [N][8], plane 1 + j = candidate j of cand [npeaks][N][3] (cand null with
// npeaks 0).  For the forward result (du, dv) of row t at grid point i (uv0 from xyuvav [N][6], as the search kernels read it):
//   no fit (du or dv not finite)                            why = kFbNoFit
//   |du| or |dv| >= 2^30, or with r = ((int)rintf(du), (int)rintf(dv)) and m = uv0 + (off_u, off_v) + r the chip of half-width ocw at m
//   leaves the H x W image                                  why = kFbLeaves
//   otherwise                                               why = kFbSearch, xy2[t] = point i's row with (u, v) = m, sh2[t] = -r
// A row that is not searched gets (u, v) = (-1, -1) and shift 0: a chip that leaves the image, which every search kernel turns into an
// all-NaN record before it reads a plane (the _dev entries' contract).
hipError_t launch_fb_seed(const double *xyuvav, int N, int off_u, int off_v, const float *out, const float *cand, int npeaks, int ocw, int H,
                          int W, double *xy2 /*[(1+npeaks) N][6]*/, int32_t *sh2 /*[(1+npeaks) N][2]*/, uint8_t *why /*[(1+npeaks) N]*/,
                          hipStream_t s);
// fb[t] = (du_b, dv_b, ncc_b, err) from the backward record back[t] (back [(1+npeaks) N][8]) and the forward (du, dv) of row t:
//   err = (float)hypot((double)du + (double)du_b, (double)dv + (double)dv_b) where du_b and dv_b are finite, NaN otherwise;
//   why[t] != kFbSearch: (NaN, NaN, -why[t], NaN).
hipError_t launch_fb_compose(const float *out, const float *cand, int N, int npeaks, const float *back, const uint8_t *why,
                             float *fb /*[(1+npeaks) N][4]*/, hipStream_t s);

}  // namespace mimc3
