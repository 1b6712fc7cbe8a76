// stack_kernel.hip -- NCC stacking (mimc3_stack_*; stack_kernel.h): stack_add_kernel accumulates one layer of surfaces into the stack's
// f64 sums and u16 counts, stack_tail_kernel forms the mean surface of every point in LDS and hands it to the tail every front of the
// exhaustive search shares (match_full_tail.h, unmodified: the record and the candidates of a stack are that text's).  Beyond R 15
// stack_tail_wide_kernel does the same with one workgroup per point and the candidate tail of match_wide_tail.h, unmodified as well.
// stack_add_scaled_kernel accumulates a layer of another time baseline: every stack cell takes the bilinear value of the layer's surface
// at scale x its displacement, times the layer's weight; a weighted stack keeps the weights' sum per cell in a third plane, wsum.
#include "stack_kernel.h"
#include "stack_acc.h"
#include "match_full_tail.h"
#include "match_wide_tail.h"

namespace mimc3 {

namespace {

// ---- the accumulation: elementwise over the chunk's flat cell array, 24 bytes of traffic per cell (4 read, 10 read and written) ------
// a point's layer count: the lane that owns the point's cell k = 0 calls this
__device__ __forceinline__ void stack_count_layer(const float *__restrict__ rec, const uint8_t *__restrict__ refused, uint32_t pt,
                                                  uint16_t *__restrict__ lay)
{
    const bool ref = (rec && rec[8 * (size_t)pt + 2] == -3.0f) || (refused && refused[pt] != 0);
    if (!ref) lay[pt] = (uint16_t)(lay[pt] + 1);
}

// Cells [head, head + 4 nvec) go four per lane (surf + head is 16-byte aligned; S^2 is odd, so a group of four may straddle two points);
// the head and the total - head - 4 nvec cells behind them, six at most, go one per lane of block 0.  wide: sum + head and cnt + head
// are 16- and 8-byte aligned as well (always so on the stack's own chunks)
__global__ __launch_bounds__(256) void stack_add_kernel(const float *__restrict__ surf, const float *__restrict__ rec,
                                                        const uint8_t *__restrict__ refused, uint32_t total, uint32_t NC, uint32_t head,
                                                        uint32_t nvec, int wide, double *__restrict__ sum, uint16_t *__restrict__ cnt,
                                                        uint16_t *__restrict__ lay, double *__restrict__ wsum)
{
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < nvec; g += stride) {
        const uint32_t i = head + 4u * g;
        const float4 v = *reinterpret_cast<const float4 *>(surf + i);
        const bool f0 = __builtin_isfinite(v.x), f1 = __builtin_isfinite(v.y), f2 = __builtin_isfinite(v.z), f3 = __builtin_isfinite(v.w);
        if (wide) {
            double2 a = *reinterpret_cast<const double2 *>(sum + i), b = *reinterpret_cast<const double2 *>(sum + i + 2);
            ushort4 c = *reinterpret_cast<const ushort4 *>(cnt + i);
            if (f0) { a.x += (double)v.x; c.x = (uint16_t)(c.x + 1); }
            if (f1) { a.y += (double)v.y; c.y = (uint16_t)(c.y + 1); }
            if (f2) { b.x += (double)v.z; c.z = (uint16_t)(c.z + 1); }
            if (f3) { b.y += (double)v.w; c.w = (uint16_t)(c.w + 1); }
            *reinterpret_cast<double2 *>(sum + i) = a;
            *reinterpret_cast<double2 *>(sum + i + 2) = b;
            *reinterpret_cast<ushort4 *>(cnt + i) = c;
            if (wsum) {                 // (a weighted stack: this layer's weight is 1; wsum + head is aligned as sum + head is)
                double2 wa = *reinterpret_cast<const double2 *>(wsum + i), wb = *reinterpret_cast<const double2 *>(wsum + i + 2);
                if (f0) wa.x += 1.0;
                if (f1) wa.y += 1.0;
                if (f2) wb.x += 1.0;
                if (f3) wb.y += 1.0;
                *reinterpret_cast<double2 *>(wsum + i) = wa;
                *reinterpret_cast<double2 *>(wsum + i + 2) = wb;
            }
        } else {
            if (f0) { sum[i] += (double)v.x; cnt[i] = (uint16_t)(cnt[i] + 1); }
            if (f1) { sum[i + 1] += (double)v.y; cnt[i + 1] = (uint16_t)(cnt[i + 1] + 1); }
            if (f2) { sum[i + 2] += (double)v.z; cnt[i + 2] = (uint16_t)(cnt[i + 2] + 1); }
            if (f3) { sum[i + 3] += (double)v.w; cnt[i + 3] = (uint16_t)(cnt[i + 3] + 1); }
            if (wsum) {
                if (f0) wsum[i] += 1.0;
                if (f1) wsum[i + 1] += 1.0;
                if (f2) wsum[i + 2] += 1.0;
                if (f3) wsum[i + 3] += 1.0;
            }
        }
        const uint32_t q = i / NC, r = i - q * NC;                // NC >= 9: at most one cell k = 0 among the four
        if (r == 0) stack_count_layer(rec, refused, q, lay);
        else if (r + 3u >= NC) stack_count_layer(rec, refused, q + 1u, lay);
    }
    if (blockIdx.x == 0 && threadIdx.x < total - 4u * nvec) {
        const uint32_t i = threadIdx.x < head ? threadIdx.x : 4u * nvec + threadIdx.x;
        const float v = surf[i];
        if (__builtin_isfinite(v)) {
            sum[i] += (double)v; cnt[i] = (uint16_t)(cnt[i] + 1);
            if (wsum) wsum[i] += 1.0;
        }
        if (i % NC == 0) stack_count_layer(rec, refused, i / NC, lay);
    }
}

// ---- a scaled and weighted layer (the definition is in include/mimc3_hip.h) -----------------------------------------------------------
// One workgroup per point.  The point's layer surface, Sl x Sl floats (36,100 bytes at Sl = 95: dynamic LDS, sized by Rl at the launch),
// is read from HBM once into LDS in its k order; then the stack's cells are walked with k contiguous over the threads, so the
// read-modify-writes of sum, cnt and wsum are coalesced.  One lane owns a cell (plain read-modify-writes), thread 0 counts lay.
// Every f64 operation below is the definition's, in its order (-ffp-contract=off: nothing fuses); stack_scaled_axis is stack_acc.h's,
// which the accumulating forms of the matrix-core searches share.
__global__ __launch_bounds__(256) void stack_add_scaled_kernel(const float *__restrict__ surf, const float *__restrict__ rec,
                                                               const uint8_t *__restrict__ refused, const int32_t *__restrict__ shift,
                                                               const int32_t *__restrict__ lshift, int R, int Rl, double s, double w,
                                                               double *__restrict__ sum, uint16_t *__restrict__ cnt,
                                                               double *__restrict__ wsum, uint16_t *__restrict__ lay)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char scaled_smem[];
    float *L = reinterpret_cast<float *>(scaled_smem);           // L[ju * Sl + jv]
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint32_t pt = blockIdx.x;                              // the grid is the launch's n points
    const int S = 2 * R + 1, NC = S * S, Sl = 2 * Rl + 1, NCl = Sl * Sl;
    const float *__restrict__ src = surf + (size_t)pt * (size_t)NCl;
    for (int j = tid; j < NCl; j += nt) L[j] = src[j];
    if (tid == 0) stack_count_layer(rec, refused, pt, lay);
    __syncthreads();
    const int32_t shu = shift[2 * (size_t)pt], shv = shift[2 * (size_t)pt + 1];
    const int32_t lu = lshift[2 * (size_t)pt], lv = lshift[2 * (size_t)pt + 1];
    const size_t base = (size_t)pt * (size_t)NC;
    for (int k = tid; k < NC; k += nt) {
        const int x = k / S, y = k - S * x;                      // su = x - R, sv = y - R
        double au, av;
        int ju, jv;
        stack_scaled_axis(s, shu, x - R, lu, Rl, au, ju);
        stack_scaled_axis(s, shv, y - R, lv, Rl, av, jv);
        const bool two_u = au != 0.0, two_v = av != 0.0;          // a tap of weight zero is not read: it may be NaN or lie outside
        if (ju < 0 || jv < 0 || ju + (two_u ? 1 : 0) >= Sl || jv + (two_v ? 1 : 0) >= Sl) continue;
        const float *l0 = L + ju * Sl + jv;
        double value = two_v ? (1.0 - av) * (double)l0[0] + av * (double)l0[1] : (double)l0[0];
        if (two_u) {
            const float *l1 = l0 + Sl;
            const double r1 = two_v ? (1.0 - av) * (double)l1[0] + av * (double)l1[1] : (double)l1[0];
            value = (1.0 - au) * value + au * r1;
        }
        if (!__builtin_isfinite(value)) continue;
        sum[base + k] += w * value;
        cnt[base + k] = (uint16_t)(cnt[base + k] + 1);
        if (wsum) wsum[base + k] += w;
    }
}

// the layer shift of every point: (int32)rint(s (double)shift), half to even (one f64 product, v_rndne_f64)
__global__ __launch_bounds__(256) void stack_layer_shift_kernel(const int32_t *__restrict__ shift, uint32_t n2, double s,
                                                                int32_t *__restrict__ lshift)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n2) lshift[i] = (int32_t)__builtin_rint(s * (double)shift[i]);
}

// the first weighted add: wsum = (double)cnt over every cell of the stack
__global__ __launch_bounds__(256) void stack_wsum_init_kernel(const uint16_t *__restrict__ cnt, size_t cells, double *__restrict__ wsum)
{
    const size_t stride = (size_t)gridDim.x * 256u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < cells; i += stride) wsum[i] = (double)cnt[i];
}

// ---- the result: one wave64 per point, four points per workgroup -------------------------------------------------------------------
template <bool MULTI_>
struct StackCfg {                       // (what match_full_tail.h asks of a configuration)
    static constexpr int VP = 33;       // pitch (words) of the surface
    static constexpr bool PEAK = false, MULTI = MULTI_;
};

constexpr int kStackWaves = 4;

template <bool MULTI>
__global__ __launch_bounds__(64 * kStackWaves) void stack_tail_kernel(MatchU8Args p, const double *__restrict__ sum,
                                                                      const uint16_t *__restrict__ cnt, const uint16_t *__restrict__ lay,
                                                                      const double *__restrict__ wsum, int min_count,
                                                                      float *__restrict__ surf, uint16_t *__restrict__ count)
{
    using C = StackCfg<MULTI>;
    __shared__ float vals[kStackWaves][32 * C::VP];              // val[y * VP + x], x, y <= 30
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gidx = blockIdx.x * kStackWaves + wave;
    const int R = p.full_R, S = 2 * R + 1, NC = S * S;
    float *val = vals[wave];
    const bool live = gidx < p.N;
    int layers = 0;
    if (live) {
        layers = lay[gidx];
        if (count && lane == 0) count[gidx] = (uint16_t)layers;
        const size_t base = (size_t)gidx * (size_t)NC;
        for (int k = lane; k < NC; k += 64) {
            const int c = cnt[base + k];
            const double d = wsum ? wsum[base + k] : (double)c;  // (a weighted stack divides by the weights' sum)
            const float m = c >= min_count ? (float)(sum[base + k] / d) : __builtin_nanf("");             // f64 division, rounded once
            const int x = k / S, y = k - S * x;
            val[y * C::VP + x] = m;
            if (surf) surf[base + k] = m;
        }
    }
    __syncthreads();                    // every wave, the ones beyond N too: the surface is in LDS before the tail reads it
    if (!live) return;
    if (layers == 0) {
        if (lane == 0) { mx::full_store(p.out + 8 * (size_t)gidx, -3.0f); mx::full_cand_fill<C>(p, gidx, -3.0f); }
        return;
    }
    const int shu = p.full_shift ? p.full_shift[2 * (size_t)gidx] : 0, shv = p.full_shift ? p.full_shift[2 * (size_t)gidx + 1] : 0;
    mx::full_tail<C>(p, val, gidx, shu, shv, lane);
    if constexpr (MULTI) mx::full_tail_multi<C>(p, val, gidx, shu, shv, lane);
}

// ---- the result beyond R 15: one workgroup of four wave64 per point --------------------------------------------------------------
// A surface of up to 95 x 95 cells does not fit a wave's share of LDS four times over, and its candidate tail (match_wide_tail.h) wants
// every wave of the workgroup for the bit plane.  The configuration is the one match_wide_kernel.hip hands the two tails: pitch 96,
// 256 threads.  Dynamic LDS, sized by R at the launch: the bit plane (kWideLmBytes), then S rows of VP words -- 37,760 bytes at S = 95,
// 13,952 at S = 33 (four and eleven workgroups per CU by LDS; the kernel streams 10 bytes per cell and is expected to follow that).
template <bool MULTI_>
struct StackWideCfg {
    static constexpr int VP = 96, NT = 256;
    static constexpr bool PEAK = false, MULTI = MULTI_;
    static constexpr int lds_bytes(int R) { return mx::kWideLmBytes + (2 * R + 1) * VP * 4; }
};
static_assert(mx::kWideLmBytes % 16 == 0, "the surface behind the bit plane stays 16-byte aligned");
static_assert(2 * kStackMaxRadius + 1 < StackWideCfg<false>::VP, "the surface pitch");
static_assert(kStackAccMaxRadius == kStackMaxRadius, "the accumulating forms of the searches take every stack (match_kernel.h)");
static_assert((2 * kStackMaxRadius + 1) * (2 * kStackMaxRadius + 1) <= 64 * 32 * mx::kWideLmWords, "the bit plane of the candidate tail");

template <bool MULTI>
__global__ __launch_bounds__(StackWideCfg<MULTI>::NT) void stack_tail_wide_kernel(MatchU8Args p, const double *__restrict__ sum,
                                                                                  const uint16_t *__restrict__ cnt,
                                                                                  const uint16_t *__restrict__ lay,
                                                                                  const double *__restrict__ wsum, int min_count,
                                                                                  float *__restrict__ surf, uint16_t *__restrict__ count)
{
    using C = StackWideCfg<MULTI>;
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_smem[];
    uint32_t *bits = reinterpret_cast<uint32_t *>(stack_smem);
    float *val = reinterpret_cast<float *>(stack_smem + mx::kWideLmBytes);       // val[y * VP + x], x, y <= 94
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gidx = blockIdx.x;                                 // the grid is N workgroups
    const int R = p.full_R, S = 2 * R + 1, NC = S * S;
    const int layers = lay[gidx];
    if (count && tid == 0) count[gidx] = (uint16_t)layers;
    const size_t base = (size_t)gidx * (size_t)NC;
    for (int k = tid; k < NC; k += C::NT) {                      // k contiguous over the threads: sum, cnt and surf are coalesced
        const int c = cnt[base + k];
        const double d = wsum ? wsum[base + k] : (double)c;      // (a weighted stack divides by the weights' sum)
        const float m = c >= min_count ? (float)(sum[base + k] / d) : __builtin_nanf("");             // f64 division, rounded once
        const int x = k / S, y = k - S * x;
        val[y * C::VP + x] = m;
        if (surf) surf[base + k] = m;
    }
    if (layers == 0) {                  // (uniform over the workgroup: nobody waits at a barrier below)
        if (tid == 0) { mx::full_store(p.out + 8 * (size_t)gidx, -3.0f); mx::full_cand_fill<C>(p, gidx, -3.0f); }
        return;
    }
    __syncthreads();                    // the surface is in LDS before any tail reads it
    if constexpr (MULTI) {
        mx::wide_lm_plane<C>(p, val, bits, tid);
        __syncthreads();
    }
    if (wave != 0) return;
    const int shu = p.full_shift ? p.full_shift[2 * (size_t)gidx] : 0, shv = p.full_shift ? p.full_shift[2 * (size_t)gidx + 1] : 0;
    mx::full_tail<C>(p, val, gidx, shu, shv, lane);
    if constexpr (MULTI) mx::wide_tail_multi<C>(p, val, bits, gidx, shu, shv, lane);
}

}  // namespace

hipError_t launch_stack_add(const float *surf, const float *rec, const uint8_t *refused, int n, int NC, double *sum, uint16_t *cnt,
                            uint16_t *lay, double *wsum, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    constexpr int kMaxNC = (2 * kStackMaxRadius + 1) * (2 * kStackMaxRadius + 1);
    if (!surf || !sum || !cnt || !lay || n > kStackChunk || NC < 9 || NC > kMaxNC || (int64_t)n * NC > kStackChunkCells)
        return hipErrorInvalidValue;
    const uint32_t total = (uint32_t)n * (uint32_t)NC;            // <= 65536 * 961 < 2^26 (stack_chunk)
    uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(surf) & 15u)) & 15u) / 4u;
    if (reinterpret_cast<uintptr_t>(surf) & 3u) return hipErrorInvalidValue;
    if (head > total) head = total;
    const uint32_t nvec = (total - head) / 4u;
    const int wide = (reinterpret_cast<uintptr_t>(sum + head) & 15u) == 0 && (reinterpret_cast<uintptr_t>(cnt + head) & 7u) == 0 &&
                     (!wsum || (reinterpret_cast<uintptr_t>(wsum + head) & 15u) == 0);
    uint32_t nb = (nvec + 255u) / 256u;
    nb = nb < 1u ? 1u : nb > 2048u ? 2048u : nb;                 // 256 CUs x 8 workgroups; the grid-stride loop takes the rest
    hipLaunchKernelGGL(stack_add_kernel, dim3(nb), dim3(256), 0, s, surf, rec, refused, total, (uint32_t)NC, head, nvec, wide, sum, cnt, lay, wsum);
    return hipGetLastError();
}

hipError_t launch_stack_add_scaled(const float *surf, const float *rec, const uint8_t *refused, const int32_t *shift, const int32_t *lshift,
                                   int n, int R, int Rl, double scale, double weight, double *sum, uint16_t *cnt, double *wsum,
                                   uint16_t *lay, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int64_t NC = (2 * R + 1) * (2 * R + 1), NCl = (2 * Rl + 1) * (2 * Rl + 1);
    if (!surf || !shift || !lshift || !sum || !cnt || !lay || R < 1 || R > kStackMaxRadius || Rl < 1 || Rl > kStackMaxRadius ||
        n * NC > kStackChunkCells || n * NCl > kStackChunkCells || !(scale >= 1.0 / 64 && scale <= 64.0) ||
        !(weight > 0.0 && __builtin_isfinite(weight)) || (reinterpret_cast<uintptr_t>(surf) & 3u))
        return hipErrorInvalidValue;
    // one wave per point where neither surface has more cells than a wave walks in 16 steps (R, Rl <= 15), four waves beyond
    const unsigned nt = (NC > NCl ? NC : NCl) <= 1024 ? 64u : 256u;
    hipLaunchKernelGGL(stack_add_scaled_kernel, dim3((unsigned)n), dim3(nt), (size_t)NCl * sizeof(float), s, surf, rec, refused, shift,
                       lshift, R, Rl, scale, weight, sum, cnt, wsum, lay);                // (below the default limit of dynamic LDS)
    return hipGetLastError();
}

hipError_t launch_stack_layer_shift(const int32_t *shift, int N, double scale, int32_t *lshift, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (!shift || !lshift) return hipErrorInvalidValue;
    const uint32_t n2 = 2u * (uint32_t)N;
    hipLaunchKernelGGL(stack_layer_shift_kernel, dim3((n2 + 255u) / 256u), dim3(256), 0, s, shift, n2, scale, lshift);
    return hipGetLastError();
}

hipError_t launch_stack_wsum_init(const uint16_t *cnt, size_t cells, double *wsum, hipStream_t s)
{
    if (cells == 0) return hipSuccess;
    if (!cnt || !wsum) return hipErrorInvalidValue;
    const size_t nb = (cells + 255u) / 256u;
    hipLaunchKernelGGL(stack_wsum_init_kernel, dim3((unsigned)(nb > 4096u ? 4096u : nb)), dim3(256), 0, s, cnt, cells, wsum);
    return hipGetLastError();
}

hipError_t launch_stack_tail(const double *sum, const uint16_t *cnt, const uint16_t *lay, const double *wsum, const int32_t *shift, int N,
                             int R, int npeaks, int min_count, float *out, float *cand, float *surf, uint16_t *count, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (!sum || !cnt || !lay || !out || R < 1 || R > kStackMaxRadius || min_count < 1 || npeaks < 0 || npeaks > kFullMaxPeaks ||
        (npeaks > 0) != (cand != nullptr))
        return hipErrorInvalidValue;
    MatchU8Args a{};
    a.out = out; a.N = N; a.full_R = R; a.full_shift = shift;
    if (cand) { a.full_cand = cand; a.full_npeaks = npeaks; }
    if (R > 15) {
        const int lds = StackWideCfg<false>::lds_bytes(R);       // (below the default limit of dynamic LDS: no attribute to set)
        if (cand) hipLaunchKernelGGL(stack_tail_wide_kernel<true>, dim3((unsigned)N), dim3(256), lds, s, a, sum, cnt, lay, wsum, min_count, surf, count);
        else hipLaunchKernelGGL(stack_tail_wide_kernel<false>, dim3((unsigned)N), dim3(256), lds, s, a, sum, cnt, lay, wsum, min_count, surf, count);
        return hipGetLastError();
    }
    const unsigned nb = (unsigned)(((size_t)N + kStackWaves - 1) / kStackWaves);
    if (cand) hipLaunchKernelGGL(stack_tail_kernel<true>, dim3(nb), dim3(64 * kStackWaves), 0, s, a, sum, cnt, lay, wsum, min_count, surf, count);
    else hipLaunchKernelGGL(stack_tail_kernel<false>, dim3(nb), dim3(64 * kStackWaves), 0, s, a, sum, cnt, lay, wsum, min_count, surf, count);
    return hipGetLastError();
}

}  // namespace mimc3
