// fb_kernel.hip -- the two elementwise kernels of the forward-backward consistency check (mimc3_match_ncc_full_fb; fb_kernel.h): one
// thread per row t = plane * N + i.  Plain loads and stores, no atomics, no LDS; under 100 bytes per row each.
#include "fb_kernel.h"

namespace mimc3 {

namespace {

// the forward (du, dv) of row t: the record's columns 0, 1 (plane 0) or candidate plane - 1's
__device__ __forceinline__ float2 fb_forward(const float *__restrict__ out, const float *__restrict__ cand, size_t N, size_t t)
{
    const float *q = t < N ? out + 8 * t : cand + 3 * (t - N);           // cand is [npeaks][N][3]: row t - N of it
    return make_float2(q[0], q[1]);
}

__global__ __launch_bounds__(256) void fb_seed_kernel(const double *__restrict__ xyuvav, size_t N, size_t rows, int off_u, int off_v,
                                                      const float *__restrict__ out, const float *__restrict__ cand, int ocw, int H, int W,
                                                      double *__restrict__ xy2, int32_t *__restrict__ sh2, uint8_t *__restrict__ why)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    const size_t i = t % N;
    const double *row = xyuvav + 6 * i;                   // (the caller's arrays: element loads, no alignment beyond the element's asked)
    const double2 a = make_double2(row[0], row[1]), b = make_double2(row[2], row[3]), c = make_double2(row[4], row[5]);   // (x, y), (u, v), (vx, vy)
    const float2 d = fb_forward(out, cand, N, t);
    uint8_t r = kFbSearch;
    int ru = 0, rv = 0;
    double mu = -1.0, mv = -1.0;
    if (!(__builtin_isfinite(d.x) && __builtin_isfinite(d.y))) r = kFbNoFit;
    else if (!(__builtin_fabsf(d.x) < 1073741824.0f && __builtin_fabsf(d.y) < 1073741824.0f)) r = kFbLeaves;
    else {
        ru = (int)rintf(d.x); rv = (int)rintf(d.y);
        const int64_t pu = (int64_t)(int)b.x + off_u + ru, pv = (int64_t)(int)b.y + off_v + rv;
        if (pu - ocw < 0 || pu + ocw >= W || pv - ocw < 0 || pv + ocw >= H) { r = kFbLeaves; ru = 0; rv = 0; }
        else { mu = (double)pu; mv = (double)pv; }
    }
    double2 *o = reinterpret_cast<double2 *>(xy2 + 6 * t);
    o[0] = a; o[1] = make_double2(mu, mv); o[2] = c;
    *reinterpret_cast<int2 *>(sh2 + 2 * t) = make_int2(-ru, -rv);
    why[t] = r;
}

__global__ __launch_bounds__(256) void fb_compose_kernel(const float *__restrict__ out, const float *__restrict__ cand, size_t N, size_t rows,
                                                         const float *__restrict__ back, const uint8_t *__restrict__ why,
                                                         float *__restrict__ fb)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    const float nan = __builtin_nanf("");
    const uint8_t r = why[t];
    float4 o;
    if (r != kFbSearch) o = make_float4(nan, nan, -(float)r, nan);
    else {
        const float4 q = *reinterpret_cast<const float4 *>(back + 8 * t);    // du_b, dv_b, ncc_b (or the backward status), -
        const float2 d = fb_forward(out, cand, N, t);
        float err = nan;
        if (__builtin_isfinite(q.x) && __builtin_isfinite(q.y))             // (two f64 additions and the library's hypot: nothing to contract)
            err = (float)hypot((double)d.x + (double)q.x, (double)d.y + (double)q.y);
        o = make_float4(q.x, q.y, q.z, err);
    }
    float *w = fb + 4 * t;
    w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = o.w;
}

}  // namespace

hipError_t launch_fb_seed(const double *xyuvav, int N, int off_u, int off_v, const float *out, const float *cand, int npeaks, int ocw, int H,
                          int W, double *xy2, int32_t *sh2, uint8_t *why, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (!xyuvav || !out || !xy2 || !sh2 || !why || npeaks < 0 || npeaks > 8 || (npeaks > 0) != (cand != nullptr)) return hipErrorInvalidValue;
    const size_t rows = (size_t)(1 + npeaks) * (size_t)N;
    hipLaunchKernelGGL(fb_seed_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, xyuvav, (size_t)N, rows, off_u, off_v, out, cand,
                       ocw, H, W, xy2, sh2, why);
    return hipGetLastError();
}

hipError_t launch_fb_compose(const float *out, const float *cand, int N, int npeaks, const float *back, const uint8_t *why, float *fb,
                             hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (!out || !back || !why || !fb || npeaks < 0 || npeaks > 8 || (npeaks > 0) != (cand != nullptr)) return hipErrorInvalidValue;
    const size_t rows = (size_t)(1 + npeaks) * (size_t)N;
    hipLaunchKernelGGL(fb_compose_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, out, cand, (size_t)N, rows, back, why, fb);
    return hipGetLastError();
}

}  // namespace mimc3
