// stack.cpp -- NCC stacking of the C ABI (mimc3_stack_*, include/mimc3_hip.h; stack_kernel.hip): the surfaces of several pairs -- each a
// mimc3_match_ncc_full_any(mode 1) layer on the pair that is resident (mimc3_stack_add_class: the same cells from the kernel of the
// pair's class), or a caller's array -- accumulated per cell in f64, and the tail
// of the exhaustive search over their mean.  The stack is state of the context that the image setters do not touch.  Every entry
// validates everything before its first launch.  A layer from the resident pair is a search of the exhaustive-search family: checked,
// selected and launched through that layer's functions (search.cpp).  mimc3_stack_add_fused takes a layer at any chip size and radius: on an
// 8-bit or scaled-integer pair the run-time-ocw matrix-core search adds every surface into the stack itself (its accumulating forms,
// stack_acc.h: no layer scratch); any other pair goes through the layer scratch as above.  mimc3_stack_add_scaled_fused is the same for a layer
// of another time baseline: the search runs at the layer's radius around the layer shift and resamples every surface into the stack.
#include <cmath>
#include <cstring>
#include "ctx_internal.h"
#include "stack_kernel.h"

using namespace mimc3;

static void stack_release(mimc3_ctx *c)
{
    auto &k = c->stk;
    for (DevBuf *b : {&k.sum, &k.cnt, &k.lay, &k.shift, &k.wsum, &k.lsh, &k.layer, &k.rec, &k.ref, &k.out, &k.cand, &k.surf, &k.count})
        b->release();
    std::vector<int32_t>().swap(k.h_shift);
    k.N = 0; k.R = 0; k.layers = 0; k.weighted = false;
}

static inline size_t stack_cells(const mimc3_ctx *c) { return (size_t)((2 * c->stk.R + 1) * (2 * c->stk.R + 1)); }
// the weights' sums from cell `cell0` on; null on a stack that is not weighted
static inline double *stack_wsum(const mimc3_ctx *c, size_t cell0)
{
    return c->stk.weighted ? static_cast<double *>(c->stk.wsum.p) + cell0 : nullptr;
}

// (max_R 15: mimc3_stack_begin; 47: mimc3_stack_begin_wide -- one text, so a stack of R <= 15 is the same state through either)
static int stack_begin(mimc3_ctx *c, int32_t N, int32_t R, const int32_t *shift, int max_R, const char *entry)
{
    const std::string en(entry);
    if (!c || N < 0) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    if (c->child) return mimc3::fail(MIMC3_ESTATE, en + ": not on a chip-atlas context");
    HIP_TRY(hipSetDevice(c->device));
    if (N == 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        stack_release(c);
        return 0;
    }
    if (R < 1 || R > max_R) return mimc3::fail(MIMC3_EINVAL, en + ": R must be in 1.." + std::to_string(max_R));
    auto &k = c->stk;
    k.N = 0; k.R = 0; k.layers = 0;                             // (no stack while this one is being sized)
    if (k.weighted || k.wsum.p) {                               // the new stack is not weighted: 10 bytes per cell again
        HIP_TRY(hipStreamSynchronize(c->stream));
        k.wsum.release();
        k.weighted = false;
    }
    const size_t NC = (size_t)((2 * R + 1) * (2 * R + 1)), cells = (size_t)N * NC;
    HIP_TRY(k.sum.reserve(sizeof(double) * cells));
    HIP_TRY(k.cnt.reserve(sizeof(uint16_t) * cells));
    HIP_TRY(k.lay.reserve(sizeof(uint16_t) * (size_t)N));
    HIP_TRY(k.shift.reserve(sizeof(int32_t) * 2 * (size_t)N));
    HIP_TRY(hipMemsetAsync(k.sum.p, 0, sizeof(double) * cells, c->stream));
    HIP_TRY(hipMemsetAsync(k.cnt.p, 0, sizeof(uint16_t) * cells, c->stream));
    HIP_TRY(hipMemsetAsync(k.lay.p, 0, sizeof(uint16_t) * (size_t)N, c->stream));
    k.h_shift.assign(2 * (size_t)N, 0);
    if (shift) {
        std::memcpy(k.h_shift.data(), shift, sizeof(int32_t) * 2 * (size_t)N);
        RC_TRY(h2d_copy(c, k.shift.p, shift, sizeof(int32_t) * 2 * (size_t)N));
    } else {
        HIP_TRY(hipMemsetAsync(k.shift.p, 0, sizeof(int32_t) * 2 * (size_t)N, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));                   // (the adds may come in on another stream)
    k.N = N; k.R = R;
    return 0;
}

extern "C" int mimc3_stack_begin(mimc3_ctx *c, int32_t N, int32_t R, const int32_t *shift)
{
    return stack_begin(c, N, R, shift, 15, "mimc3_stack_begin");
}

extern "C" int mimc3_stack_begin_wide(mimc3_ctx *c, int32_t N, int32_t R, const int32_t *shift)
{
    return stack_begin(c, N, R, shift, mimc3::kStackMaxRadius, "mimc3_stack_begin_wide");
}

extern "C" int32_t mimc3_stack_chunk(int32_t R) { return mimc3::stack_chunk(R); }

extern "C" int mimc3_stack_info(mimc3_ctx *c, int32_t *N, int32_t *R, int32_t *layers)
{
    if (!c) return mimc3::fail(MIMC3_EINVAL, "mimc3_stack_info: bad argument");
    if (N) *N = c->stk.N;
    if (R) *R = c->stk.R;
    if (layers) *layers = c->stk.layers;
    return 0;
}

// what every add checks about the stack itself
static int stack_add_state(mimc3_ctx *c, int32_t N, const std::string &en)
{
    if (c->child) return mimc3::fail(MIMC3_ESTATE, en + ": not on a chip-atlas context");
    if (c->stk.N == 0) return mimc3::fail(MIMC3_ESTATE, en + ": no stack (mimc3_stack_begin)");
    if (N != c->stk.N) return mimc3::fail(MIMC3_EINVAL, en + ": N differs from the stack's");
    if (c->stk.layers >= 65535) return mimc3::fail(MIMC3_ESTATE, en + ": the stack holds 65,535 layers");
    return 0;
}

// a layer of a stack beyond R 15 is mimc3_match_ncc_wide's: the chip size must take the stack's radius (ocw is one of the six)
static int stack_add_radius(mimc3_ctx *c, int32_t ocw, const std::string &en)
{
    if (c->stk.R > 15 && c->stk.R > mimc3::wide_max_radius(ocw))
        return mimc3::fail(MIMC3_EINVAL, en + ": the stack's R exceeds mimc3_wide_max_radius(ocw)");
    return 0;
}

// A layer from the resident pair is a search in mode 1 -- the float kernel, the wide one beyond R 15 -- that returns its surfaces: what
// an add shares with the search (its arguments, the chip size, the images) is the search's to refuse; the radius is the stack's.
// A class layer (mimc3_stack_add_class) is the same search in mode 0 with the surfaces from whichever kernel runs: the kernel of the
// pair's class up to R 15 -- the same cells, so the same state -- and the wide kernel beyond, which is mimc3_stack_add itself
static const SearchRules kLayerRules = {kFloat, false, true, kCandAbsent, false, false, true};
static const SearchRules kClassLayerRules = {kFloat, false, true, kCandAbsent, false, false, true, true};
static int layer_check(mimc3_ctx *c, const char *entry, const double *xyuvav, int32_t N, int32_t ocw, bool host, bool cls = false)
{
    SearchCall call{};
    call.entry = entry; call.host = host; call.d_xyuvav = xyuvav; call.N = N; call.ocw = ocw; call.mode = cls ? 0 : 1;
    return search_check(c, call, cls ? kClassLayerRules : kLayerRules);
}
// the search of one chunk of a layer at radius R around `d_shift`: records into `rec`, surfaces into `layer`
static SearchCall layer_call(const char *entry, const double *d_xyuvav, int32_t n, int32_t off_u, int32_t off_v, const int32_t *d_shift,
                             int32_t ocw, int32_t R, int32_t swap, float *rec, float *layer, hipStream_t s, bool cls = false)
{
    return SearchCall{entry, false, d_xyuvav, 6, 2, n, off_u, off_v, d_shift, ocw, R, 0, swap ? 1 : 0, cls ? 0 : 1, 0, rec, nullptr, layer, nullptr, nullptr, s};
}

// A checked layer through the layer scratch: the search `rules` select for `call` (its R the stack's, its points, shifts, records and
// surfaces set per chunk here) in chunks of mimc3_stack_chunk(R) points, each followed by stack_add_kernel over its surfaces and records
static int stack_add_chunked(mimc3_ctx *c, const double *d_xyuvav, int32_t N, SearchCall call, const SearchRules &rules)
{
    auto &k = c->stk;
    const size_t NC = stack_cells(c);
    const size_t chunk = (size_t)(N < mimc3::stack_chunk(k.R) ? N : mimc3::stack_chunk(k.R));
    hipStream_t s = call.stream;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(k.layer.reserve(sizeof(float) * chunk * NC));
    HIP_TRY(k.rec.reserve(sizeof(float) * 8 * chunk));
    float *layer = static_cast<float *>(k.layer.p), *rec = static_cast<float *>(k.rec.p);
    call.d_out = rec; call.d_surf = layer;
    SearchKernel kernel;
    PlaneSet planes;
    RC_TRY(pick_kernel(c, call, rules, kernel));
    RC_TRY(plane_set(c, kernel, 0, planes));                    // (planes a first call builds: on the context's stream, which it drains)
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    TimingSuspended whole(c);           // (the events bracket the whole call)
    for (size_t g0 = 0; g0 < (size_t)N; g0 += chunk) {
        call.N = (int32_t)((size_t)N - g0 < chunk ? (size_t)N - g0 : chunk);
        call.d_xyuvav = d_xyuvav + 6 * g0;
        call.d_shift = static_cast<const int32_t *>(k.shift.p) + 2 * g0;
        RC_TRY(launch_search(c, kernel, planes, call));
        const hipError_t e = mimc3::launch_stack_add(layer, rec, nullptr, call.N, (int)NC, static_cast<double *>(k.sum.p) + g0 * NC,
                                                     static_cast<uint16_t *>(k.cnt.p) + g0 * NC, static_cast<uint16_t *>(k.lay.p) + g0,
                                                     stack_wsum(c, g0 * NC), s);
        if (e != hipSuccess) return mimc3::hip_fail(e, "stack add kernel launch");
    }
    k.layers++;
    if (whole.was) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

static int stack_add_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t swap,
                         void *stream, const char *entry, bool cls)
{
    const std::string en(entry);
    // the search's refusals and the stack's own, before anything is allocated or enqueued
    RC_TRY(layer_check(c, entry, d_xyuvav, N, ocw, false, cls));
    RC_TRY(stack_add_state(c, N, en));
    RC_TRY(stack_add_radius(c, ocw, en));
    const SearchCall call = layer_call(entry, d_xyuvav, 0, off_u, off_v, static_cast<const int32_t *>(c->stk.shift.p), ocw, c->stk.R, swap, nullptr,
                                       nullptr, static_cast<hipStream_t>(stream), cls);
    return stack_add_chunked(c, d_xyuvav, N, call, cls ? kClassLayerRules : kLayerRules);
}

extern "C" int mimc3_stack_add_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t swap,
                                   void *stream)
{
    return stack_add_dev(c, d_xyuvav, N, off_u, off_v, ocw, swap, stream, "mimc3_stack_add_dev", false);
}

extern "C" int mimc3_stack_add_class_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                                         int32_t swap, void *stream)
{
    return stack_add_dev(c, d_xyuvav, N, off_u, off_v, ocw, swap, stream, "mimc3_stack_add_class_dev", true);
}

static int stack_add_host(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap, const char *entry,
                          bool cls)
{
    const std::string en(entry);
    if (!offset) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(layer_check(c, entry, xyuvav, N, ocw, true, cls));
    RC_TRY(stack_add_state(c, N, en));
    RC_TRY(stack_add_radius(c, ocw, en));
    // the chip inside the image, the search box inside the planes' zero border (as mimc3_match_ncc_full_any's host entry)
    RC_TRY(search_check_host(c, entry, xyuvav, N, offset, c->stk.h_shift.data(), ocw, c->stk.R));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->xy.reserve(sizeof(double) * 6 * (size_t)N));
    RC_TRY(h2d_copy(c, c->xy.p, xyuvav, sizeof(double) * 6 * (size_t)N));
    RC_TRY(stack_add_dev(c, static_cast<const double *>(c->xy.p), N, offset[0], offset[1], ocw, swap, c->stream, entry, cls));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mimc3_stack_add(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap)
{
    return stack_add_host(c, xyuvav, N, offset, ocw, swap, "mimc3_stack_add", false);
}

extern "C" int mimc3_stack_add_class(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap)
{
    return stack_add_host(c, xyuvav, N, offset, ocw, swap, "mimc3_stack_add_class", true);
}

// ---- a layer at any chip size and radius, accumulated in the matrix-core search's own tail (mimc3_stack_add_fused; the definition is
//      in include/mimc3_hip.h).  The layer is mimc3_match_ncc_wide_planes(mode 0, surf)'s: that entry's rules, as a layer ----
static const SearchRules kFusedRules = {kFloat, true, false, kCandAbsent, false, false, true, false, true, true, true, true, true};
static int fused_check(mimc3_ctx *c, const char *entry, const double *xyuvav, int32_t N, int32_t ocw, bool host)
{
    SearchCall call{};
    call.entry = entry; call.host = host; call.d_xyuvav = xyuvav; call.N = N; call.ocw = ocw;
    return search_check(c, call, kFusedRules);
}
// The largest stack radius the entry takes for the resident pair's class at a valid ocw: the matrix-core wide kernels' own on an 8-bit
// and on a scaled-integer pair; on any other pair what mimc3_match_ncc_wide_planes(mode 0) takes -- the float wide kernel at the six,
// R 15 elsewhere
static int fused_max_radius(mimc3_ctx *c, int32_t ocw, PairClass &cls, int32_t &lim)
{
    RC_TRY(pair_class(c, cls));
    const int32_t w = full_ocw_ok(ocw) ? mimc3::wide_max_radius(ocw) : 0;
    lim = cls == kU8 ? mimc3::wide_u8_max_radius(ocw) : cls == kScaledInt ? mimc3::wide_u16_max_radius(ocw) : w > 15 ? w : 15;
    return 0;
}

extern "C" int32_t mimc3_stack_fused_max_radius(mimc3_ctx *c, int32_t ocw)
{
    if (!c || ocw < 1 || ocw > mimc3::kFullChipMaxOcw || !c->d_i0 || !c->d_i1 || c->child) return 0;
    PairClass cls;
    int32_t lim = 0;
    return fused_max_radius(c, ocw, cls, lim) ? 0 : lim;
}

static int stack_add_fused_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t swap,
                               void *stream, const char *entry)
{
    const std::string en(entry);
    // the search's refusals, the stack's own and the radius, before anything is allocated, enqueued or counted
    RC_TRY(fused_check(c, entry, d_xyuvav, N, ocw, false));
    RC_TRY(stack_add_state(c, N, en));
    auto &k = c->stk;
    PairClass cls;
    int32_t lim = 0;
    RC_TRY(fused_max_radius(c, ocw, cls, lim));
    if (k.R > lim)
        return mimc3::fail(MIMC3_EINVAL, en + ": the stack's R exceeds mimc3_stack_fused_max_radius(ctx, ocw) = " + std::to_string(lim));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SearchCall call = layer_call(entry, d_xyuvav, N, off_u, off_v, static_cast<const int32_t *>(k.shift.p), ocw, k.R, swap, nullptr, nullptr, s, true);
    // any other class: what mimc3_match_ncc_wide_planes(mode 0, surf) runs, through the layer scratch
    if (cls != kU8 && cls != kScaledInt) return stack_add_chunked(c, d_xyuvav, N, call, kFusedRules);
    // the accumulating forms: one search over all N points that adds every finished surface into the stack itself
    const SearchKernel kernel = cls == kU8 ? (k.R <= 15 ? ChipU8 : WideU8) : (k.R <= 15 ? ChipU16 : WideU16);
    call.stk_sum = static_cast<double *>(k.sum.p); call.stk_cnt = static_cast<uint16_t *>(k.cnt.p);
    call.stk_lay = static_cast<uint16_t *>(k.lay.p); call.stk_wsum = stack_wsum(c, 0);
    PlaneSet planes;
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(plane_set(c, kernel, 0, planes));                    // (planes a first call builds: on the context's stream, which it drains)
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    TimingSuspended whole(c);           // (the events bracket the whole call)
    RC_TRY(launch_search(c, kernel, planes, call));
    k.layers++;
    if (whole.was) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

extern "C" int mimc3_stack_add_fused_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                                         int32_t swap, void *stream)
{
    return stack_add_fused_dev(c, d_xyuvav, N, off_u, off_v, ocw, swap, stream, "mimc3_stack_add_fused_dev");
}

extern "C" int mimc3_stack_add_fused(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap)
{
    const char *entry = "mimc3_stack_add_fused";
    const std::string en(entry);
    if (!offset) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(fused_check(c, entry, xyuvav, N, ocw, true));
    RC_TRY(stack_add_state(c, N, en));
    PairClass cls;
    int32_t lim = 0;
    RC_TRY(fused_max_radius(c, ocw, cls, lim));
    if (c->stk.R > lim)
        return mimc3::fail(MIMC3_EINVAL, en + ": the stack's R exceeds mimc3_stack_fused_max_radius(ctx, ocw) = " + std::to_string(lim));
    // the chip inside the image, the search box inside the planes' zero border (as mimc3_stack_add)
    RC_TRY(search_check_host(c, entry, xyuvav, N, offset, c->stk.h_shift.data(), ocw, c->stk.R));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->xy.reserve(sizeof(double) * 6 * (size_t)N));
    RC_TRY(h2d_copy(c, c->xy.p, xyuvav, sizeof(double) * 6 * (size_t)N));
    RC_TRY(stack_add_fused_dev(c, static_cast<const double *>(c->xy.p), N, offset[0], offset[1], ocw, swap, c->stream, entry));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mimc3_stack_add_surfaces_dev(mimc3_ctx *c, const float *d_surf, const uint8_t *d_refused, int32_t N, void *stream)
{
    const std::string en("mimc3_stack_add_surfaces_dev");
    if (!c || !d_surf || N <= 0 || (reinterpret_cast<uintptr_t>(d_surf) & 3u)) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(stack_add_state(c, N, en));
    auto &k = c->stk;
    const size_t NC = stack_cells(c), chunk = (size_t)mimc3::stack_chunk(k.R);
    HIP_TRY(hipSetDevice(c->device));
    for (size_t g0 = 0; g0 < (size_t)N; g0 += chunk) {
        const int n = (int)((size_t)N - g0 < chunk ? (size_t)N - g0 : chunk);
        const hipError_t e = mimc3::launch_stack_add(d_surf + g0 * NC, nullptr, d_refused ? d_refused + g0 : nullptr, n, (int)NC,
                                                     static_cast<double *>(k.sum.p) + g0 * NC, static_cast<uint16_t *>(k.cnt.p) + g0 * NC,
                                                     static_cast<uint16_t *>(k.lay.p) + g0, stack_wsum(c, g0 * NC),
                                                     static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return mimc3::hip_fail(e, "stack add kernel launch");
    }
    k.layers++;
    return 0;
}

extern "C" int mimc3_stack_add_surfaces(mimc3_ctx *c, const float *surf, const uint8_t *refused, int32_t N)
{
    const std::string en("mimc3_stack_add_surfaces");
    if (!c || !surf || N <= 0) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(stack_add_state(c, N, en));
    auto &k = c->stk;
    const size_t NC = stack_cells(c);
    const size_t chunk = (size_t)(N < mimc3::stack_chunk(k.R) ? N : mimc3::stack_chunk(k.R));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(k.layer.reserve(sizeof(float) * chunk * NC));
    if (refused) {
        HIP_TRY(k.ref.reserve((size_t)N));
        RC_TRY(h2d_copy(c, k.ref.p, refused, (size_t)N));
    }
    // one chunk of surfaces at a time through the layer scratch; copies and launches are ordered on the context's stream
    for (size_t g0 = 0; g0 < (size_t)N; g0 += chunk) {
        const int n = (int)((size_t)N - g0 < chunk ? (size_t)N - g0 : chunk);
        RC_TRY(h2d_copy(c, k.layer.p, surf + g0 * NC, sizeof(float) * (size_t)n * NC));
        const hipError_t e = mimc3::launch_stack_add(static_cast<const float *>(k.layer.p), nullptr,
                                                     refused ? static_cast<const uint8_t *>(k.ref.p) + g0 : nullptr, n, (int)NC,
                                                     static_cast<double *>(k.sum.p) + g0 * NC, static_cast<uint16_t *>(k.cnt.p) + g0 * NC,
                                                     static_cast<uint16_t *>(k.lay.p) + g0, stack_wsum(c, g0 * NC), c->stream);
        if (e != hipSuccess) return mimc3::hip_fail(e, "stack add kernel launch");
    }
    k.layers++;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- layers of another time baseline: scaled and weighted (the definition is in include/mimc3_hip.h) ----
static inline bool stack_scale_ok(double s) { return s >= 1.0 / 64 && s <= 64.0; }                // (false for NaN)
static inline bool stack_weight_ok(double w) { return w > 0.0 && std::isfinite(w); }

extern "C" int32_t mimc3_stack_layer_radius(int32_t R, double scale)
{
    if (R < 1 || R > mimc3::kStackMaxRadius || !stack_scale_ok(scale)) return 0;
    return scale == 1.0 ? R : (int32_t)std::floor(scale * (double)R + 0.5) + 1;
}

// the layer shift of every point from the stack's host shift; MIMC3_EINVAL where |scale shift| >= 2^30.  out may be null (the check alone)
static int stack_layer_shift(const mimc3_ctx *c, double scale, int32_t *out, const std::string &en)
{
    const std::vector<int32_t> &sh = c->stk.h_shift;
    for (size_t i = 0; i < sh.size(); ++i) {
        const double p = scale * (double)sh[i];
        if (!(std::fabs(p) < 1073741824.0)) return mimc3::fail(MIMC3_EINVAL, en + ": |scale x shift| must be below 2^30");
        if (out) out[i] = (int32_t)std::nearbyint(p);           // (half to even: the default rounding mode, which nothing here changes)
    }
    return 0;
}

// what every scaled add checks beyond its pointers, before anything is allocated or enqueued
static int stack_scaled_check(mimc3_ctx *c, int32_t N, int32_t layer_R, int32_t max_R, double scale, double weight, const std::string &en)
{
    RC_TRY(stack_add_state(c, N, en));
    if (!stack_scale_ok(scale)) return mimc3::fail(MIMC3_EINVAL, en + ": scale must be in 1/64..64");
    if (!stack_weight_ok(weight)) return mimc3::fail(MIMC3_EINVAL, en + ": weight must be finite and > 0");
    if (layer_R < 1 || layer_R > max_R)
        return mimc3::fail(MIMC3_EINVAL, en + ": layer_R must be in 1.." + std::to_string(max_R));
    return stack_layer_shift(c, scale, nullptr, en);
}

extern "C" int mimc3_stack_layer_shift(mimc3_ctx *c, double scale, int32_t *out)
{
    const std::string en("mimc3_stack_layer_shift");
    if (!c || !out) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    if (c->stk.N == 0) return mimc3::fail(MIMC3_ESTATE, en + ": no stack (mimc3_stack_begin)");
    if (!stack_scale_ok(scale)) return mimc3::fail(MIMC3_EINVAL, en + ": scale must be in 1/64..64");
    return stack_layer_shift(c, scale, out, en);
}

extern "C" int mimc3_stack_weighted(mimc3_ctx *c) { return c && c->stk.N != 0 && c->stk.weighted ? 1 : 0; }

// the points of one launch of a scaled add: neither the layer's slice nor the stack's exceeds kStackChunkCells
static inline size_t stack_scaled_chunk(const mimc3_ctx *c, int32_t N, int32_t layer_R)
{
    const int a = mimc3::stack_chunk(c->stk.R), b = mimc3::stack_chunk(layer_R);
    const int m = a < b ? a : b;
    return (size_t)(N < m ? N : m);
}

// What a scaled add enqueues on `s` before its first chunk: the wsum plane of a stack that this add makes weighted, and the layer shift.
// Called after every check has passed.
static int stack_scaled_prepare(mimc3_ctx *c, double scale, double weight, hipStream_t s)
{
    auto &k = c->stk;
    const size_t cells = (size_t)k.N * stack_cells(c);
    HIP_TRY(k.lsh.reserve(sizeof(int32_t) * 2 * (size_t)k.N));
    if (weight != 1.0 && !k.weighted) {
        HIP_TRY(k.wsum.reserve(sizeof(double) * cells));
        const hipError_t e = mimc3::launch_stack_wsum_init(static_cast<const uint16_t *>(k.cnt.p), cells, static_cast<double *>(k.wsum.p), s);
        if (e != hipSuccess) return mimc3::hip_fail(e, "stack wsum kernel launch");
        k.weighted = true;
    }
    const hipError_t e = mimc3::launch_stack_layer_shift(static_cast<const int32_t *>(k.shift.p), k.N, scale, static_cast<int32_t *>(k.lsh.p), s);
    if (e != hipSuccess) return mimc3::hip_fail(e, "stack layer-shift kernel launch");
    return 0;
}

// A checked scaled layer through the layer scratch: the search `rules` select for `call` (its R the layer's; its points, layer shifts,
// records and surfaces set per chunk here) in chunks of min(mimc3_stack_chunk(R), mimc3_stack_chunk(layer_R)) points, each followed by
// stack_add_scaled_kernel over its surfaces and records
static int stack_add_scaled_chunked(mimc3_ctx *c, const double *d_xyuvav, int32_t N, SearchCall call, const SearchRules &rules, double scale,
                                    double weight)
{
    auto &k = c->stk;
    const int32_t layer_R = call.R;
    const size_t NC = stack_cells(c), NCl = (size_t)((2 * layer_R + 1) * (2 * layer_R + 1));
    const size_t chunk = stack_scaled_chunk(c, N, layer_R);
    hipStream_t s = call.stream;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(k.layer.reserve(sizeof(float) * chunk * NCl));
    HIP_TRY(k.rec.reserve(sizeof(float) * 8 * chunk));
    float *layer = static_cast<float *>(k.layer.p), *rec = static_cast<float *>(k.rec.p);
    call.d_out = rec; call.d_surf = layer;
    SearchKernel kernel;
    PlaneSet planes;
    RC_TRY(pick_kernel(c, call, rules, kernel));
    RC_TRY(plane_set(c, kernel, 0, planes));                    // (as mimc3_stack_add_dev)
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    TimingSuspended whole(c);           // (the events bracket the whole call)
    RC_TRY(stack_scaled_prepare(c, scale, weight, s));
    for (size_t g0 = 0; g0 < (size_t)N; g0 += chunk) {
        const int32_t n = (int32_t)((size_t)N - g0 < chunk ? (size_t)N - g0 : chunk);
        const int32_t *lsh = static_cast<const int32_t *>(k.lsh.p) + 2 * g0;
        call.N = n; call.d_xyuvav = d_xyuvav + 6 * g0; call.d_shift = lsh;
        RC_TRY(launch_search(c, kernel, planes, call));
        const hipError_t e = mimc3::launch_stack_add_scaled(layer, rec, nullptr, static_cast<const int32_t *>(k.shift.p) + 2 * g0, lsh, n, k.R,
                                                            layer_R, scale, weight, static_cast<double *>(k.sum.p) + g0 * NC,
                                                            static_cast<uint16_t *>(k.cnt.p) + g0 * NC, stack_wsum(c, g0 * NC),
                                                            static_cast<uint16_t *>(k.lay.p) + g0, s);
        if (e != hipSuccess) return mimc3::hip_fail(e, "scaled stack add kernel launch");
    }
    k.layers++;
    if (whole.was) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

static int stack_add_scaled_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t layer_R,
                                int32_t swap, double scale, double weight, void *stream, const char *entry)
{
    const std::string en(entry);
    RC_TRY(layer_check(c, entry, d_xyuvav, N, ocw, false));
    RC_TRY(stack_scaled_check(c, N, layer_R, mimc3::wide_max_radius(ocw), scale, weight, en));
    // mimc3_match_ncc_wide(npeaks 0, shift = the layer shift, R = layer_R, surf): the float kernel up to 15, the wide kernel beyond
    const SearchCall call = layer_call(entry, d_xyuvav, 0, off_u, off_v, nullptr, ocw, layer_R, swap, nullptr, nullptr, static_cast<hipStream_t>(stream));
    return stack_add_scaled_chunked(c, d_xyuvav, N, call, kLayerRules, scale, weight);
}

extern "C" int mimc3_stack_add_scaled_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                                          int32_t layer_R, int32_t swap, double scale, double weight, void *stream)
{
    return stack_add_scaled_dev(c, d_xyuvav, N, off_u, off_v, ocw, layer_R, swap, scale, weight, stream, "mimc3_stack_add_scaled_dev");
}

extern "C" int mimc3_stack_add_scaled(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t layer_R,
                                      int32_t swap, double scale, double weight)
{
    const char *entry = "mimc3_stack_add_scaled";
    const std::string en(entry);
    if (!offset) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(layer_check(c, entry, xyuvav, N, ocw, true));
    RC_TRY(stack_scaled_check(c, N, layer_R, mimc3::wide_max_radius(ocw), scale, weight, en));
    // the chip inside the image, the layer's search box inside the planes' zero border (as mimc3_stack_add, around the layer shift)
    std::vector<int32_t> lsh(c->stk.h_shift.size());
    RC_TRY(stack_layer_shift(c, scale, lsh.data(), en));
    RC_TRY(search_check_host(c, entry, xyuvav, N, offset, lsh.data(), ocw, layer_R));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->xy.reserve(sizeof(double) * 6 * (size_t)N));
    RC_TRY(h2d_copy(c, c->xy.p, xyuvav, sizeof(double) * 6 * (size_t)N));
    RC_TRY(stack_add_scaled_dev(c, static_cast<const double *>(c->xy.p), N, offset[0], offset[1], ocw, layer_R, swap, scale, weight,
                                c->stream, entry));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- a scaled layer at any chip size and layer radius, resampled in the matrix-core search's own tail (mimc3_stack_add_scaled_fused; the
//      definition is in include/mimc3_hip.h).  The layer is mimc3_match_ncc_wide_planes(mode 0, surf)'s around the layer shift ----
// what both entries check beyond the search's refusals, before anything is allocated, enqueued or counted: the stack's own, then the
// scale, the weight, the layer radius against mimc3_stack_fused_max_radius(ctx, ocw) and the layer shift's range
static int stack_scaled_fused_check(mimc3_ctx *c, int32_t N, int32_t ocw, int32_t layer_R, double scale, double weight, PairClass &cls,
                                    const std::string &en)
{
    RC_TRY(stack_add_state(c, N, en));
    int32_t lim = 0;
    RC_TRY(fused_max_radius(c, ocw, cls, lim));
    return stack_scaled_check(c, N, layer_R, lim, scale, weight, en);
}

static int stack_add_scaled_fused_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                                      int32_t layer_R, int32_t swap, double scale, double weight, void *stream, const char *entry)
{
    const std::string en(entry);
    PairClass cls;
    RC_TRY(fused_check(c, entry, d_xyuvav, N, ocw, false));
    RC_TRY(stack_scaled_fused_check(c, N, ocw, layer_R, scale, weight, cls, en));
    auto &k = c->stk;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SearchCall call = layer_call(entry, d_xyuvav, N, off_u, off_v, nullptr, ocw, layer_R, swap, nullptr, nullptr, s, true);
    // any other class: what mimc3_match_ncc_wide_planes(mode 0, surf) runs, through the layer scratch and stack_add_scaled_kernel
    if (cls != kU8 && cls != kScaledInt) return stack_add_scaled_chunked(c, d_xyuvav, N, call, kFusedRules, scale, weight);
    // the accumulating forms: one search over all N points, every workgroup resampling its finished surface into the stack itself
    const SearchKernel kernel = cls == kU8 ? (layer_R <= 15 ? ChipU8 : WideU8) : (layer_R <= 15 ? ChipU16 : WideU16);
    PlaneSet planes;
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(plane_set(c, kernel, 0, planes));                    // (planes a first call builds: on the context's stream, which it drains)
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    TimingSuspended whole(c);           // (the events bracket the whole call)
    RC_TRY(stack_scaled_prepare(c, scale, weight, s));          // (the wsum plane of a stack this add makes weighted; the layer shift)
    call.d_shift = static_cast<const int32_t *>(k.lsh.p);
    call.stk_sum = static_cast<double *>(k.sum.p); call.stk_cnt = static_cast<uint16_t *>(k.cnt.p);
    call.stk_lay = static_cast<uint16_t *>(k.lay.p); call.stk_wsum = stack_wsum(c, 0);
    call.stk_shift = static_cast<const int32_t *>(k.shift.p); call.stk_R = k.R; call.stk_scale = scale; call.stk_weight = weight;
    RC_TRY(launch_search(c, kernel, planes, call));
    k.layers++;
    if (whole.was) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

extern "C" int mimc3_stack_add_scaled_fused_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                                                int32_t layer_R, int32_t swap, double scale, double weight, void *stream)
{
    return stack_add_scaled_fused_dev(c, d_xyuvav, N, off_u, off_v, ocw, layer_R, swap, scale, weight, stream, "mimc3_stack_add_scaled_fused_dev");
}

extern "C" int mimc3_stack_add_scaled_fused(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw,
                                            int32_t layer_R, int32_t swap, double scale, double weight)
{
    const char *entry = "mimc3_stack_add_scaled_fused";
    const std::string en(entry);
    if (!offset) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    PairClass cls;
    RC_TRY(fused_check(c, entry, xyuvav, N, ocw, true));
    RC_TRY(stack_scaled_fused_check(c, N, ocw, layer_R, scale, weight, cls, en));
    // the chip inside the image, the layer's search box inside the planes' zero border (as mimc3_stack_add_scaled)
    std::vector<int32_t> lsh(c->stk.h_shift.size());
    RC_TRY(stack_layer_shift(c, scale, lsh.data(), en));
    RC_TRY(search_check_host(c, entry, xyuvav, N, offset, lsh.data(), ocw, layer_R));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->xy.reserve(sizeof(double) * 6 * (size_t)N));
    RC_TRY(h2d_copy(c, c->xy.p, xyuvav, sizeof(double) * 6 * (size_t)N));
    RC_TRY(stack_add_scaled_fused_dev(c, static_cast<const double *>(c->xy.p), N, offset[0], offset[1], ocw, layer_R, swap, scale, weight,
                                      c->stream, entry));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mimc3_stack_add_surfaces_scaled_dev(mimc3_ctx *c, const float *d_surf, const uint8_t *d_refused, int32_t N, int32_t layer_R,
                                                   double scale, double weight, void *stream)
{
    const std::string en("mimc3_stack_add_surfaces_scaled_dev");
    if (!c || !d_surf || N <= 0 || (reinterpret_cast<uintptr_t>(d_surf) & 3u)) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(stack_scaled_check(c, N, layer_R, mimc3::kStackMaxRadius, scale, weight, en));
    auto &k = c->stk;
    const size_t NC = stack_cells(c), NCl = (size_t)((2 * layer_R + 1) * (2 * layer_R + 1)), chunk = stack_scaled_chunk(c, N, layer_R);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(stack_scaled_prepare(c, scale, weight, s));
    for (size_t g0 = 0; g0 < (size_t)N; g0 += chunk) {
        const int n = (int)((size_t)N - g0 < chunk ? (size_t)N - g0 : chunk);
        const hipError_t e = mimc3::launch_stack_add_scaled(d_surf + g0 * NCl, nullptr, d_refused ? d_refused + g0 : nullptr,
                                                            static_cast<const int32_t *>(k.shift.p) + 2 * g0,
                                                            static_cast<const int32_t *>(k.lsh.p) + 2 * g0, n, k.R, layer_R, scale, weight,
                                                            static_cast<double *>(k.sum.p) + g0 * NC, static_cast<uint16_t *>(k.cnt.p) + g0 * NC,
                                                            stack_wsum(c, g0 * NC), static_cast<uint16_t *>(k.lay.p) + g0, s);
        if (e != hipSuccess) return mimc3::hip_fail(e, "scaled stack add kernel launch");
    }
    k.layers++;
    return 0;
}

extern "C" int mimc3_stack_add_surfaces_scaled(mimc3_ctx *c, const float *surf, const uint8_t *refused, int32_t N, int32_t layer_R,
                                               double scale, double weight)
{
    const std::string en("mimc3_stack_add_surfaces_scaled");
    if (!c || !surf || N <= 0) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    RC_TRY(stack_scaled_check(c, N, layer_R, mimc3::kStackMaxRadius, scale, weight, en));
    auto &k = c->stk;
    const size_t NC = stack_cells(c), NCl = (size_t)((2 * layer_R + 1) * (2 * layer_R + 1)), chunk = stack_scaled_chunk(c, N, layer_R);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(k.layer.reserve(sizeof(float) * chunk * NCl));
    if (refused) {
        HIP_TRY(k.ref.reserve((size_t)N));
        RC_TRY(h2d_copy(c, k.ref.p, refused, (size_t)N));
    }
    RC_TRY(stack_scaled_prepare(c, scale, weight, c->stream));
    // one chunk of surfaces at a time through the layer scratch; copies and launches are ordered on the context's stream
    for (size_t g0 = 0; g0 < (size_t)N; g0 += chunk) {
        const int n = (int)((size_t)N - g0 < chunk ? (size_t)N - g0 : chunk);
        RC_TRY(h2d_copy(c, k.layer.p, surf + g0 * NCl, sizeof(float) * (size_t)n * NCl));
        const hipError_t e = mimc3::launch_stack_add_scaled(static_cast<const float *>(k.layer.p), nullptr,
                                                            refused ? static_cast<const uint8_t *>(k.ref.p) + g0 : nullptr,
                                                            static_cast<const int32_t *>(k.shift.p) + 2 * g0,
                                                            static_cast<const int32_t *>(k.lsh.p) + 2 * g0, n, k.R, layer_R, scale, weight,
                                                            static_cast<double *>(k.sum.p) + g0 * NC, static_cast<uint16_t *>(k.cnt.p) + g0 * NC,
                                                            stack_wsum(c, g0 * NC), static_cast<uint16_t *>(k.lay.p) + g0, c->stream);
        if (e != hipSuccess) return mimc3::hip_fail(e, "scaled stack add kernel launch");
    }
    k.layers++;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

static int stack_finish_check(mimc3_ctx *c, int32_t npeaks, int32_t min_count, const float *out, const float *cand, const std::string &en)
{
    if (!c || !out) return mimc3::fail(MIMC3_EINVAL, en + ": bad argument");
    if (npeaks < 0 || npeaks > mimc3::kFullMaxPeaks) return mimc3::fail(MIMC3_EINVAL, en + ": npeaks must be in 0..8");
    if ((npeaks == 0) != (cand == nullptr)) return mimc3::fail(MIMC3_EINVAL, en + ": cand goes with npeaks > 0");
    if (min_count < 1 || min_count > 65535) return mimc3::fail(MIMC3_EINVAL, en + ": min_count must be in 1..65535");
    if (c->stk.N == 0) return mimc3::fail(MIMC3_ESTATE, en + ": no stack (mimc3_stack_begin)");
    return 0;
}

extern "C" int mimc3_stack_finish_dev(mimc3_ctx *c, int32_t npeaks, int32_t min_count, float *d_out, float *d_cand, float *d_surf,
                                      uint16_t *d_count, void *stream)
{
    RC_TRY(stack_finish_check(c, npeaks, min_count, d_out, d_cand, "mimc3_stack_finish_dev"));
    auto &k = c->stk;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    const hipError_t e = mimc3::launch_stack_tail(static_cast<const double *>(k.sum.p), static_cast<const uint16_t *>(k.cnt.p),
                                                  static_cast<const uint16_t *>(k.lay.p), stack_wsum(c, 0),
                                                  static_cast<const int32_t *>(k.shift.p), k.N, k.R, npeaks, min_count, d_out, d_cand,
                                                  d_surf, d_count, s);
    if (e != hipSuccess) return mimc3::hip_fail(e, "stack tail kernel launch");
    if (c->timing) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

extern "C" int mimc3_stack_finish(mimc3_ctx *c, int32_t npeaks, int32_t min_count, float *out, float *cand, float *surf, uint16_t *count)
{
    RC_TRY(stack_finish_check(c, npeaks, min_count, out, cand, "mimc3_stack_finish"));
    auto &k = c->stk;
    const size_t N = (size_t)k.N, NC = stack_cells(c);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(k.out.reserve(sizeof(float) * 8 * N));
    if (npeaks) HIP_TRY(k.cand.reserve(sizeof(float) * 3 * (size_t)npeaks * N));
    if (surf) HIP_TRY(k.surf.reserve(sizeof(float) * N * NC));
    if (count) HIP_TRY(k.count.reserve(sizeof(uint16_t) * N));
    RC_TRY(mimc3_stack_finish_dev(c, npeaks, min_count, static_cast<float *>(k.out.p), npeaks ? static_cast<float *>(k.cand.p) : nullptr,
                                  surf ? static_cast<float *>(k.surf.p) : nullptr, count ? static_cast<uint16_t *>(k.count.p) : nullptr,
                                  c->stream));
    RC_TRY(d2h_copy(c, out, k.out.p, sizeof(float) * 8 * N));
    if (npeaks) RC_TRY(d2h_copy(c, cand, k.cand.p, sizeof(float) * 3 * (size_t)npeaks * N));
    if (surf) RC_TRY(d2h_copy(c, surf, k.surf.p, sizeof(float) * N * NC));
    if (count) RC_TRY(d2h_copy(c, count, k.count.p, sizeof(uint16_t) * N));
    return 0;
}
