// pyramid_kernel.hip -- the small kernels of the coarse-to-fine exhaustive search (mimc3_match_ncc_pyramid / _pyramid_dn, capi.cpp): the
// 2 x 2 null-aware reduction that makes one pyramid level of a plane (one kernel per plane type: u8, u16, f32, and f32 of any float
// pair for mimc3_match_ncc_pyramid_any), and the per-point step that carries the search centre from one level to the next.  The searches
// themselves are the full mode of the matrix-core kernel (match_mx_kernel.hip) and the register-tiled full kernels
// (match_full_u16_kernel.hip, match_full_f32_kernel.hip, match_full_f32g_kernel.hip).
#include "match_kernel.h"

namespace mimc3 {

namespace {

// one output pixel from its 2 x 2 block (the bytes a, b of the top row, c, d of the bottom row): the rounded mean of the non-zero ones
__device__ __forceinline__ uint32_t reduce4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t n = (a != 0u) + (b != 0u) + (c != 0u) + (d != 0u);
    return n ? (a + b + c + d + (n >> 1)) / n : 0u;
}

// lane (j, y): destination pixels x = 4 j .. 4 j + 3 of row y -- two dwords of each of the two source rows in, one dword out.  Every
// offset is a multiple of 4 (pad and the pitches are), and the columns x >= Wd of the last dword are written as zeros (the border).
__global__ __launch_bounds__(256) void pyr_reduce_kernel(const unsigned char *__restrict__ src, int Wps, unsigned char *__restrict__ dst, int Hd,
                                                         int Wd, int Wpd, int pad)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (4 * j >= Wd || y >= Hd) return;
    const uint32_t *r0 = reinterpret_cast<const uint32_t *>(src + (size_t)(2 * y + pad) * Wps + pad) + 2 * j;
    const uint32_t *r1 = reinterpret_cast<const uint32_t *>(reinterpret_cast<const unsigned char *>(r0) + Wps);
    const uint2 t = make_uint2(r0[0], r0[1]), b = make_uint2(r1[0], r1[1]);
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t tw = i < 2 ? t.x : t.y, bw = i < 2 ? b.x : b.y, sh = 16 * (i & 1);
        const uint32_t v = reduce4((tw >> sh) & 255u, (tw >> (sh + 8)) & 255u, (bw >> sh) & 255u, (bw >> (sh + 8)) & 255u);
        if (4 * j + i < Wd) o |= v << (8 * i);
    }
    *reinterpret_cast<uint32_t *>(dst + (size_t)(y + pad) * Wpd + pad + 4 * j) = o;
}

// The same reduction on the u16 plane of a scaled-integer image (q = pixel * 2^s < 4096; the level keeps s): lane (j, y) makes destination
// pixels x = 4 j .. 4 j + 3 of row y from 16 bytes of each of the two source rows (as two 8-byte halves: the pitch is a whole number of
// 8 bytes) and writes 8 bytes.  The rounded mean of values below 4096 stays below 4096.
__global__ __launch_bounds__(256) void pyr_reduce_u16_kernel(const unsigned short *__restrict__ src, int Wps, unsigned short *__restrict__ dst,
                                                             int Hd, int Wd, int Wpd, int pad)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (4 * j >= Wd || y >= Hd) return;
    const uint2 *r0 = reinterpret_cast<const uint2 *>(src + (size_t)(2 * y + pad) * Wps + pad) + 2 * j;
    const uint2 *r1 = reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned short *>(r0) + Wps);
    const uint2 ta = r0[0], tb = r0[1], ba = r1[0], bb = r1[1];
    const uint32_t t[4] = {ta.x, ta.y, tb.x, tb.y}, b[4] = {ba.x, ba.y, bb.x, bb.y};    // dword i: the block of destination pixel i
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = 4 * j + i < Wd ? reduce4(t[i] & 0xffffu, t[i] >> 16, b[i] & 0xffffu, b[i] >> 16) : 0u;
    *reinterpret_cast<uint2 *>(dst + (size_t)(y + pad) * Wpd + pad + 4 * j) = make_uint2(v[0] | v[1] << 16, v[2] | v[3] << 16);
}

// ... and on the f32 plane of an integral-f32 image (w = pixel * 2^s an integer below 2^20; mul = 2^s, inv = 2^-s): lane (j, y) makes
// destination pixels x = 2 j, 2 j + 1 from 16 bytes of each of the two source rows.  Every step is exact: the product by a power of
// two, the conversion of an integer below 2^20, the integer mean (a sum below 2^22), the conversion back and the product by 2^-s.
__global__ __launch_bounds__(256) void pyr_reduce_f32_kernel(const float *__restrict__ src, int Wps, float *__restrict__ dst, int Hd, int Wd,
                                                             int Wpd, int pad, float mul, float inv)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (2 * j >= Wd || y >= Hd) return;
    const float4 *r0 = reinterpret_cast<const float4 *>(src + (size_t)(2 * y + pad) * Wps + pad) + j;
    const float4 *r1 = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(r0) + Wps);
    const float4 t = r0[0], b = r1[0];
    const uint32_t v0 = reduce4((uint32_t)(t.x * mul), (uint32_t)(t.y * mul), (uint32_t)(b.x * mul), (uint32_t)(b.y * mul));
    const uint32_t v1 = reduce4((uint32_t)(t.z * mul), (uint32_t)(t.w * mul), (uint32_t)(b.z * mul), (uint32_t)(b.w * mul));
    *reinterpret_cast<float2 *>(dst + (size_t)(y + pad) * Wpd + pad + 2 * j) =
        make_float2((float)v0 * inv, 2 * j + 1 < Wd ? (float)v1 * inv : 0.0f);
}

// ... and on the f32 plane of ANY float pair (mimc3_match_ncc_pyramid_any): the f64 mean of the block's INCLUDED pixels, those with
// (double)p >= MIN_DN -- the reference's inclusion rule: NaN, 0, negatives and positives below 1e-10 stay out -- added in the order
// (2y, 2x), (2y, 2x + 1), (2y + 1, 2x), (2y + 1, 2x + 1) and rounded to f32 once; the canonical null 0 when none is included (an all-NaN
// block too).  Every term is selected, not multiplied by its mask: 0 * Inf and NaN must not reach the sum through an excluded pixel.
__device__ __forceinline__ float reduce4g(float a, float b, float c, float d)
{
    const double v[4] = {(double)a, (double)b, (double)c, (double)d};
    double s = 0.0;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const bool in = v[i] >= 1e-10;
        s += in ? v[i] : 0.0;                   // (s >= 0: adding 0 leaves its bits alone)
        n += in ? 1 : 0;
    }
    return n ? (float)(s / (double)n) : 0.0f;
}

// lane (j, y): destination pixels x = 2 j, 2 j + 1 from 16 bytes of each of the two source rows, as pyr_reduce_f32_kernel
__global__ __launch_bounds__(256) void pyr_reduce_f32g_kernel(const float *__restrict__ src, int Wps, float *__restrict__ dst, int Hd, int Wd,
                                                              int Wpd, int pad)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (2 * j >= Wd || y >= Hd) return;
    const float4 *r0 = reinterpret_cast<const float4 *>(src + (size_t)(2 * y + pad) * Wps + pad) + j;
    const float4 *r1 = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(r0) + Wps);
    const float4 t = r0[0], b = r1[0];
    *reinterpret_cast<float2 *>(dst + (size_t)(y + pad) * Wpd + pad + 2 * j) =
        make_float2(reduce4g(t.x, t.y, b.x, b.y), 2 * j + 1 < Wd ? reduce4g(t.z, t.w, b.z, b.w) : 0.0f);
}

__global__ __launch_bounds__(256) void pyr_step_kernel(const double *__restrict__ xyuvav, int N, int off_u, int off_v, const int32_t *shift,
                                                       const int32_t *__restrict__ peak, int R, int lnext, int first, int32_t *sh,
                                                       double *__restrict__ pos)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    int64_t du, dv;                          // (sh may be the caller's shift: each lane reads its own entry before it writes it)
    if (first) {
        du = (int64_t)off_u + (shift ? shift[2 * (size_t)g] : 0);
        dv = (int64_t)off_v + (shift ? shift[2 * (size_t)g + 1] : 0);
        if (lnext > 0) {                     // floor((D + 2^(L-2)) / 2^(L-1)), L - 1 = lnext
            const int64_t h = (int64_t)1 << (lnext - 1);
            du = (du + h) >> lnext;
            dv = (dv + h) >> lnext;
        }
    } else {
        du = sh[2 * (size_t)g];
        dv = sh[2 * (size_t)g + 1];
        const int k = peak[g], S = 2 * R + 1;
        if (k >= 0) { du += k / S - R; dv += k % S - R; }
        du *= 2;
        dv *= 2;
    }
    if (lnext == 0) { du -= off_u; dv -= off_v; }
    sh[2 * (size_t)g] = (int32_t)du;
    sh[2 * (size_t)g + 1] = (int32_t)dv;
    if (lnext > 0) {
        const double *row = xyuvav + 6 * (size_t)g;
        pos[2 * (size_t)g] = (double)((int)row[2] >> lnext);
        pos[2 * (size_t)g + 1] = (double)((int)row[3] >> lnext);
    }
}

}  // namespace

hipError_t launch_pyr_reduce(const unsigned char *src, int Hs, int Ws, int Wps, unsigned char *dst, int Hd, int Wd, int Wpd, int pad,
                             hipStream_t s)
{
    // (the last dword of a row reaches 3 pixels and its source 6 pixels past the image: inside the border)
    if (Hd < 1 || Wd < 1 || Hd > Hs / 2 || Wd > Ws / 2 || pad < 8 || (pad & 3) || (Wps & 3) || (Wpd & 3) || Wps < Ws + 2 * pad || Wpd < Wd + 2 * pad)
        return hipErrorInvalidValue;
    const int nj = (Wd + 3) / 4;
    hipLaunchKernelGGL(pyr_reduce_kernel, dim3((unsigned)((nj + 255) / 256), (unsigned)Hd), dim3(256), 0, s, src, Wps, dst, Hd, Wd, Wpd, pad);
    return hipGetLastError();
}

hipError_t launch_pyr_reduce_u16(const unsigned short *src, int Hs, int Ws, int Wps, unsigned short *dst, int Hd, int Wd, int Wpd, int pad,
                                 hipStream_t s)
{
    // (the last 8 bytes of a row reach 3 pixels and their source 6 pixels past the image: inside the border)
    if (Hd < 1 || Wd < 1 || Hd > Hs / 2 || Wd > Ws / 2 || pad < 8 || (pad & 3) || (Wps & 3) || (Wpd & 3) || Wps < Ws + 2 * pad || Wpd < Wd + 2 * pad)
        return hipErrorInvalidValue;
    const int nj = (Wd + 3) / 4;
    hipLaunchKernelGGL(pyr_reduce_u16_kernel, dim3((unsigned)((nj + 255) / 256), (unsigned)Hd), dim3(256), 0, s, src, Wps, dst, Hd, Wd, Wpd, pad);
    return hipGetLastError();
}

hipError_t launch_pyr_reduce_f32(const float *src, int Hs, int Ws, int Wps, float *dst, int Hd, int Wd, int Wpd, int pad, int shift,
                                 hipStream_t s)
{
    // (the last 8 bytes of a row reach 1 pixel and their source 2 pixels past the image: inside the border)
    if (Hd < 1 || Wd < 1 || Hd > Hs / 2 || Wd > Ws / 2 || pad < 8 || (pad & 3) || (Wps & 3) || (Wpd & 3) || Wps < Ws + 2 * pad || Wpd < Wd + 2 * pad ||
        shift < 0 || shift > 3)
        return hipErrorInvalidValue;
    const int nj = (Wd + 1) / 2;
    const float mul = (float)(1 << shift);
    hipLaunchKernelGGL(pyr_reduce_f32_kernel, dim3((unsigned)((nj + 255) / 256), (unsigned)Hd), dim3(256), 0, s, src, Wps, dst, Hd, Wd, Wpd, pad,
                       mul, 1.0f / mul);
    return hipGetLastError();
}

hipError_t launch_pyr_reduce_f32g(const float *src, int Hs, int Ws, int Wps, float *dst, int Hd, int Wd, int Wpd, int pad, hipStream_t s)
{
    // (the last 8 bytes of a row reach 1 pixel and their source 2 pixels past the image: inside the border)
    if (Hd < 1 || Wd < 1 || Hd > Hs / 2 || Wd > Ws / 2 || pad < 8 || (pad & 3) || (Wps & 3) || (Wpd & 3) || Wps < Ws + 2 * pad || Wpd < Wd + 2 * pad)
        return hipErrorInvalidValue;
    const int nj = (Wd + 1) / 2;
    hipLaunchKernelGGL(pyr_reduce_f32g_kernel, dim3((unsigned)((nj + 255) / 256), (unsigned)Hd), dim3(256), 0, s, src, Wps, dst, Hd, Wd, Wpd, pad);
    return hipGetLastError();
}

hipError_t launch_pyr_step(const double *xyuvav, int N, int off_u, int off_v, const int32_t *shift, const int32_t *peak, int R, int lnext,
                           bool first, int32_t *sh, double *pos, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (lnext < 0 || lnext > 4 || (!first && !peak) || (lnext > 0 && !pos)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pyr_step_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, xyuvav, N, off_u, off_v, shift, peak, R, lnext,
                       first ? 1 : 0, sh, pos);
    return hipGetLastError();
}

}  // namespace mimc3
