// u8_classify_kernel.hip -- which kernel takes which grid point of a DLC matcher call on an 8-bit pair, decided once per call.
//
// The matrix-core kernel (match_mx_kernel.hip) takes a point whose pivot set fits its 32 x 32 cell tile and whose chip and window hold
// no null pixel; the register-tiled kernel (match_px_kernel.hip) takes the rest.  All of that follows from the point's pivots and two
// table queries, so it is evaluated here by one thread per point -- with the helpers the matrix-core kernel's header uses
// (mx_tile_fit, mx_takes, mx_null_class in match_kernel.h; the packed tables of sat_kernel.h) -- instead of by a 128-thread workgroup
// per point that has already issued its first tile and chip loads.  Two launches:
//   u8_classify_count   the class byte of every point (this store replaces the memset of the bytes) and, per block of 256 points,
//                       how many are clean (class 0) and how many are the register-tiled kernel's (kMxRest); zeroes the overflow counter
//                       -- and the point's record (U8PointRec, match_kernel.h: everything read and derived here that the matcher kernels'
//                       headers would read and derive again) into a staging array, by point index
//   u8_classify_fill    the two index lists in ascending point order: a block sums the counts of the blocks before it (a few hundred
//                       words), ranks its own points by ballot, and writes them -- the index and, moved from the staging array, the
//                       record at the same list position; the last block writes the two list lengths
// A third list rides along: the advance list -- the REST-LIST POSITIONS of the rest points that mx_takes, whose chip is null-free and whose
// window holds nulls, but none in the climb area (mx_climb_area, match_kernel.h: one more table query).  The matrix-core launch tries
// them behind its clean list and marks those it finishes in their rest records; counted and ranked like the other two.
// A clean point's record carries its climb area too (clean_area; no query, its window holds no null): the matrix-core kernel's clean
// form finishes the NCC of the area's row bands alone.
// No same-address atomic per point (100,000 of them serialise into a millisecond) and no spinning on another block: the order inside
// both lists is the point order, whatever the order the blocks run in.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_kernel.h"
#include "sat_kernel.h"

namespace mimc3 {

namespace {

constexpr int kClsThreads = 256, kClsWaves = kClsThreads / 64;

// the point's class, and in `r` everything that was read and derived on the way: the header of the kernel that takes the point
__device__ __forceinline__ uint8_t classify_point(const MatchU8Args &p, int g, U8PointRec &r, bool advance_on, bool clean_area, bool &adv)
{
    const int OCW = p.ocw, CW = 2 * OCW + 1, PAD = p.pad;
    typedef unsigned long long SatT;
    const SatT *sat_chip = reinterpret_cast<const SatT *>(p.swap ? p.sat1 : p.sat0);
    const SatT *sat_win = reinterpret_cast<const SatT *>(p.swap ? p.sat0 : p.sat1);
    // the loads that depend on nothing but g go out together, the chip's query (as the matrix-core header issues it for every point it
    // meets) behind the point row and beside the last pivot: three memory round trips per point, not four
    const int64_t pbeg = p.piv_off[g];
    const int npiv = (int)(p.piv_off[g + 1] - pbeg);
    const double *row = p.xyuvav + (size_t)p.xy_stride * (size_t)g + p.xy_col;
    const int u0 = (int)row[0], v0 = (int)row[1];
    int2 last = make_int2(0, 0);
    if (npiv >= 1) last = *reinterpret_cast<const int2 *>(p.piv_uv + 2 * (pbeg + npiv - 1));      // (no pivot: nothing to read the search area from)
    const int cu0 = u0 - OCW + PAD, cv0 = v0 - OCW + PAD;
    const SatT chipQ = sat_box(sat_chip, p.sat_ws, cu0, cv0, CW, CW);
    const int chip_nulls = (int)(chipQ >> kSatNullShift8);
    const int lu = last.x, lv = last.y;
    const int dx2 = (lu < 0 ? -lu : lu) + OCW + 2, dy2 = (lv < 0 ? -lv : lv) + OCW + 2;
    const int csx = 2 * dx2 + 1 - 2 * OCW + 1, csy = 2 * dy2 + 1 - 2 * OCW + 1;
    int tx0, ty0;
    const bool fits = mx_tile_fit(lu, lv, OCW, dx2, dy2, csx, csy, 1, tx0, ty0);
    // the window's written area (its last row and column are never written, MIMC_module.c:869-886): the register-tiled kernel's header
    // wants its null count of every point, so it is no longer skipped for the points the tests above already send there
    const int win_nulls = sat_nulls_u8_thread(sat_win, p.sat_ws, u0 + p.off_u - dx2 + PAD, v0 + p.off_v - dy2 + PAD, 2 * dx2, 2 * dy2);
    const uint8_t cls = mx_takes(npiv, fits) ? mx_null_class(win_nulls, chip_nulls, p.mx_wn_on, p.mx_gen_on) : kMxRest;
    // the advance list: a rest point the matrix-core kernel could take but for nulls in its window (none in its chip), whose climb area
    // (mx_climb_area) holds none -- one more query.  The clean form tries it before the register-tiled launch, with its scans kept
    // inside the area; the point keeps its class and its place on the rest list
    adv = false;
    uint32_t area = kMxAreaTile;
    if (advance_on && cls == kMxRest && mx_takes(npiv, fits) && chip_nulls == 0 && win_nulls > 0) {
        int ab[4], ax, ay, aw, ah;
        mx_climb_area(lu, lv, OCW, dx2, dy2, csx, csy, tx0, ty0, ab, ax, ay, aw, ah);
        if (sat_nulls_u8_thread(sat_win, p.sat_ws, u0 + p.off_u - dx2 + PAD + ax, v0 + p.off_v - dy2 + PAD + ay, aw, ah) == 0) { adv = true; area = mx_area_pack(ab); }
    }
    // a clean point carries its climb area too (no query: its window holds no null): the clean form finishes the NCC of the area's row
    // bands alone, and a climb that leaves the area goes to the rest list as one that leaves the tile does
    if (clean_area && cls == 0) {
        int ab[4], ax, ay, aw, ah;
        mx_climb_area(lu, lv, OCW, dx2, dy2, csx, csy, tx0, ty0, ab, ax, ay, aw, ah);
        area = mx_area_pack(ab);
    }
    r.g = g; r.u0 = u0; r.v0 = v0; r.lu = lu; r.lv = lv; r.npiv = (int32_t)((uint32_t)npiv | area); r.pbeg = pbeg;
    r.win_nulls = win_nulls; r.chipQ = chipQ; r.colQ = 0; r.rowQ = 0;
    uint32_t corner = 0;
    if (cls == 0 || adv) {     // the clean form's closed-form T4 terms: the chip's last column, last row and corner pixel
        const unsigned char *chip_pl = p.swap ? p.p1 : p.p0;
        r.colQ = sat_box(sat_chip, p.sat_ws, cu0 + CW - 1, cv0, 1, CW);
        r.rowQ = sat_box(sat_chip, p.sat_ws, cu0, cv0 + CW - 1, CW, 1);
        corner = chip_pl[(size_t)(cv0 + CW - 1) * p.Wp + cu0 + CW - 1];
    }
    r.tile = (uint32_t)tx0 | (uint32_t)ty0 << 10 | (fits ? 1u << 20 : 0u) | corner << 24;
    return cls;
}
__device__ __forceinline__ void rec_copy(U8PointRec *dst, const U8PointRec *src)
{
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint4 a = s[0], b = s[1], c = s[2], e = s[3];
    d[0] = a; d[1] = b; d[2] = c; d[3] = e;
}

// the block's number of set predicates, in every thread (wave ballots, one LDS word per wave); *before = those of the lower threads
__device__ __forceinline__ int block_rank(bool on, int *wsum, int *before)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(on);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int total = 0, lower = 0;
#pragma unroll
    for (int w = 0; w < kClsWaves; w++) { const int c = wsum[w]; total += c; lower += w < wave ? c : 0; }
    *before = lower + __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kClsThreads) void u8_classify_count(MatchU8Args p, int32_t *blk, U8PointRec *stage, uint8_t *advf, bool clean_area)
{
    __shared__ int wsum[kClsWaves];
    const int g = blockIdx.x * kClsThreads + threadIdx.x;
    uint8_t cls = 0xff;
    bool adv = false;
    if (g < p.N) {
        U8PointRec r;
        cls = classify_point(p, g, r, advf != nullptr, clean_area, adv);
        p.mx_flags[g] = cls;
        if (stage) rec_copy(stage + g, &r);
        if (advf) advf[g] = adv ? 1 : 0;
    }
    int before;
    const int nclean = block_rank(cls == 0, wsum, &before);
    const int nrest = block_rank(cls == kMxRest, wsum, &before);
    const int nadv = block_rank(adv, wsum, &before);
    if (threadIdx.x == 0) {
        blk[3 * blockIdx.x] = nclean; blk[3 * blockIdx.x + 1] = nrest; blk[3 * blockIdx.x + 2] = nadv;
        if (blockIdx.x == 0) *p.ovf_count = 0;
    }
}

__global__ __launch_bounds__(kClsThreads) void u8_classify_fill(MatchU8Args p, const int32_t *blk, int32_t *lists, const U8PointRec *stage, const uint8_t *advf)
{
    __shared__ int wsum[kClsWaves];
    __shared__ int base[3];
    const int g = blockIdx.x * kClsThreads + threadIdx.x;
    if (threadIdx.x < 3) base[threadIdx.x] = 0;
    __syncthreads();
    {   // the counts of the blocks before this one
        int c0 = 0, c1 = 0, c2 = 0;
        for (int b = threadIdx.x; b < (int)blockIdx.x; b += kClsThreads) { c0 += blk[3 * b]; c1 += blk[3 * b + 1]; c2 += blk[3 * b + 2]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64); }
        if ((threadIdx.x & 63) == 0 && (c0 | c1 | c2)) { atomicAdd(&base[0], c0); atomicAdd(&base[1], c1); atomicAdd(&base[2], c2); }      // (LDS, integer: any order gives the same sum)
    }
    __syncthreads();
    const int b0 = base[0], b1 = base[1], b2 = base[2];
    const uint8_t cls = g < p.N ? p.mx_flags[g] : 0xff;
    const bool adv = advf && g < p.N && advf[g] != 0;
    int *clean = lists + kU8ListHead, *rest = lists + kU8ListHead + (size_t)p.N, *advance = lists + kU8ListHead + 2 * (size_t)p.N;
    int r;
    const int nclean = block_rank(cls == 0, wsum, &r);
    if (cls == 0) { clean[b0 + r] = g; if (stage) rec_copy(p.point_recs + (b0 + r), stage + g); }
    const int nrest = block_rank(cls == kMxRest, wsum, &r);
    if (cls == kMxRest) { rest[b1 + r] = g; if (stage) rec_copy(p.rest_recs + (b1 + r), stage + g); }
    int ra;
    const int nadv = block_rank(adv, wsum, &ra);
    if (adv) advance[b2 + ra] = b1 + r;                      // (an advance point is a rest point: its rest-list position)
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { lists[0] = b0 + nclean; lists[1] = b1 + nrest; lists[2] = b2 + nadv; }
}

}  // namespace

static inline unsigned classify_blocks(int N) { return (unsigned)((N + kClsThreads - 1) / kClsThreads); }

// per block three counts, and behind them a byte per point: it is on the advance list
static inline size_t scratch_count_ints(int N) { return 3 * (size_t)classify_blocks(N); }
size_t u8_classify_scratch_ints(int N) { return scratch_count_ints(N) + ((size_t)N + 3) / 4; }

// the records sit behind the lists and the classifier's scratch, on a 64-byte boundary: [N] clean, [N] rest, [N] staging (by point index)
static inline size_t recs_offset_ints(int N) { return (kU8ListHead + 3 * (size_t)N + u8_classify_scratch_ints(N) + 15) & ~(size_t)15; }
size_t u8_lists_bytes(int N) { return sizeof(int32_t) * recs_offset_ints(N) + 3 * (size_t)N * sizeof(U8PointRec); }
U8PointRec *u8_list_recs(int32_t *lists, int N) { return reinterpret_cast<U8PointRec *>(lists + recs_offset_ints(N)); }

hipError_t launch_u8_classify(const MatchU8Args &a, int32_t *lists, bool advance, bool clean_area, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!a.mx_flags || !a.sat0 || !a.sat1 || !a.ovf_count || !lists || !a.piv_uv || !a.piv_off) return hipErrorInvalidValue;
    if ((a.point_recs != nullptr) != (a.rest_recs != nullptr) || (a.point_recs && !a.p0)) return hipErrorInvalidValue;
    int32_t *blk = lists + kU8ListHead + 3 * (size_t)a.N;
    U8PointRec *stage = a.point_recs ? u8_list_recs(lists, a.N) + 2 * (size_t)a.N : nullptr;
    // the advance list needs the records (the clean form reads an advance point's header from its rest record); null = the list is empty
    uint8_t *advf = (advance && stage) ? reinterpret_cast<uint8_t *>(blk + scratch_count_ints(a.N)) : nullptr;
    const unsigned nb = classify_blocks(a.N);
    hipLaunchKernelGGL(u8_classify_count, dim3(nb), dim3(kClsThreads), 0, stream, a, blk, stage, advf, clean_area && stage != nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(u8_classify_fill, dim3(nb), dim3(kClsThreads), 0, stream, a, static_cast<const int32_t *>(blk), lists, static_cast<const U8PointRec *>(stage),
                       static_cast<const uint8_t *>(advf));
    return hipGetLastError();
}

}  // namespace mimc3
