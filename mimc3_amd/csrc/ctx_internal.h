// ctx_internal.h -- the context and the host helpers that capi.cpp, search.cpp and stack.cpp share (internal; host code only: never
// included by a .hip file).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/mimc3_hip.h"
#include "host_util.h"
#include "match_kernel.h"

namespace mimc3 {
int hip_fail(hipError_t e, const char *what);       // records "<what>: <HIP's text>" and returns the code of a HIP failure
}

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) return mimc3::hip_fail(e_, #expr);             \
    } while (0)
#define RC_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

// growable device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // owned: a context's buffers go with the context (mimc3_ctx_destroy selects the device first), so a member added later cannot be
    // forgotten there
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
};

// One pyramid level of a plane pair: zero-bordered planes (kU8Pad border, prepare_pair's pitch rule) and the tables of the pair's
// class -- sat of every integer class, sz (null counts) of the u16 planes alone; the float levels have neither (an unused DevBuf never
// allocates)
struct PyrLevel { DevBuf pl0, pl1, sat0, sat1, sz0, sz1; int32_t H = 0, W = 0, Wp = 0; };

struct mimc3_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // owned; host-buffer entry points run here
    const float *d_i0 = nullptr, *d_i1 = nullptr;
    DevBuf own_i0, own_i1;              // used when images were uploaded from the host
    int32_t H = 0, W = 0;
    // The pair's plane sets, one builder each (prepare_pair, build_u8_tables, build_u16, build_f32).  A builder works on `stream` and
    // drains it before it sets its ready flag, so a set is complete whatever stream a matcher call comes in on.
    DevBuf pl0, pl1, flag;              // zero-bordered u8 planes (exact-integer path) + the device tests' flags
    DevBuf sat0, sat1, sat_tmp;         // packed summed-area tables of pl0 / pl1 (sum b | sum b^2 | nulls; sat_kernel.hip), built with the planes
    DevBuf hsat0, hsat1, hsz0, hsz1;    // the same for the u16 planes hpl0 / hpl1: sum q | sum q^2, and the null counts
    bool sat_u8_ok = false, sat_u16_ok = false;   // tables hold the CURRENT planes (chip-atlas contexts build them only if a call needs them)
    DevBuf ovf;                         // [0] count, [1..] indices of points the u8 kernel handed back
    DevBuf fail;                        // [0] count, [1..] points the offset-u8 kernel handed to the u16 kernel
    bool u8o_ok = false;                // integer (shift 0) u16 planes whose local range mostly fits 8 bits: try PxU8o first
    DevBuf hpl0, hpl1;                  // zero-bordered u16 planes of scaled integers (q = value * 2^shift < 4096)
    DevBuf rt0, rt1;                    // PxU8o: min | max << 16 of every 16x16-pixel tile of hpl0 / hpl1 (valid while u8o_ok)
    bool u16_ok = false;                // the pair is scaled-integer (and not 8-bit): its u16 planes are built with the classification
    bool hpl_valid = false;             // u16 planes hold the CURRENT pair
    int shift0 = 0, shift1 = 0;         // scaled integers: pixel x 2^shift is the u16 plane's value (0 for an 8-bit pair)
    DevBuf fpl0, fpl1;                  // zero-bordered f32 planes (register-tiled f32 kernel), built on first use
    bool fplanes_ok = false;
    DevBuf fsat0, fsat1;                // their 16-byte summed-area tables when every pixel (x 1 or x 8) is an integer in [0, 2^20) (16-bit DN and its filtered forms)
    bool f32i_ok = false;
    int fshift0 = 0, fshift1 = 0;      // pixel x 2^shift is the integer the table sums
    int32_t Wp = 0;
    bool u8_ok = false;                 // both images proven to be integers in [0,255]: the u8 planes are built with the classification
    int path_mode = 0;                  // 0 auto, 1 force the general f32 kernel, 2 no integer kernels, 3 no u8 kernel, 4 auto without the matrix-core kernel
    int last_path = -1;                 // 0 general f32/f64 kernel, 1 exact u8 kernel, ... (mimc3_hip.h), 5 matrix-core u8 kernel, 9 float search kernel, 10 wide float search kernel
    DevBuf xy, puv, poff, out;          // matcher staging for the host-buffer entry point
    DevBuf pcor, pcnt, pext;            // device pivots: corridors [N] x 24 B, counts [N], extents + total (24 B)
    hipEvent_t ev_chunk[2][8] = {};     // mimc3_match_ncc_dlc_cor: "chunk uploaded + counted" / "chunk matched"
    DevBuf qm_io, qm_work;              // QM staging / workspace
    DevBuf n1_io, n1_work;              // clustering / dpf0 / dpf1 staging and workspace
    const float *raw_i0 = nullptr, *raw_i1 = nullptr;   // the pair as handed over (before any pre-filter)
    DevBuf filt0, filt1, conv_io;       // pre-filtered pair (mimc3_ctx_filter_images), conv2 staging
    DevBuf cp_buf;                      // control-point stage: one arena carved per call
    DevBuf cp_pre;                      // control-point stage: the filtered planes of a whole segment (their minima are settled before the slices start)
    bool filt_live = false;             // filt0/filt1 hold the output planes of an earlier filter pass on this pair
    hipStream_t side[3] = {nullptr, nullptr, nullptr};   // CP stage: its 16 small matcher launches per segment overlap on 4 streams
    hipEvent_t ev_side[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t aux[4] = {nullptr, nullptr, nullptr, nullptr};   // mimc3_ctx_aux_stream: copy streams of the drivers' host threads
    bool child = false;                 // a control-point child context: no streams / children of its own beyond `stream`
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // host -> device staging: two pinned chunks that a pageable source is pipelined through (a pinned source is DMA'd directly)
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t ev_pin[2] = {nullptr, nullptr};
    void *hslot[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // mimc3_ctx_host_workspace: pinned host scratch
    size_t hslot_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf slot[24];                    // mimc3_ctx_workspace: named scratch the drivers built on the ABI keep across calls
    DevBuf ovf_alt[3], fail_alt[3];     // the overflow lists of matcher lanes 1..3: calls on different streams of one context must not share them
    DevBuf mxl[4];                      // matrix-core kernel: one class byte per grid point (one buffer per lane)
    DevBuf u8l[4];                      // u8_classify: the clean and rest lists of a call with their counts (int32; one buffer per lane)
    mimc3_ctx *cp_child[4] = {nullptr, nullptr, nullptr, nullptr};   // CP stage: one context per image variant for its chip atlas (planes, kernel selection)
    DevBuf cellws;                      // general matcher: global cell-grid workspace for corridors whose cell grid outgrows LDS
    DevBuf raw_dn;                      // raw 8/16-bit DN as uploaded (mimc3_ctx_set_images_u8/_u16), widened on the device
    // coarse-to-fine search (mimc3_match_ncc_pyramid*, search.cpp): levels 1..4 of the CURRENT pair, built on first use by build_levels.
    // pyr: the levels of the pair's integer class (u8, u16 or integral-f32 planes with that class's tables) -- a pair has one class, so
    // one array serves all three.  pyrg: the float levels of the f32 planes (mimc3_match_ncc_pyramid_any; planes alone) -- mode 1 on an
    // integer-class pair builds them beside that class's levels, and both stay valid until the pair changes
    PyrLevel pyr[4], pyrg[4];
    int pyr_levels = 0, pyrg_levels = 0;
    DevBuf pyr_pos, pyr_peak, pyr_sh;   // per point: position on the level (f64 [N][2]), arg-max cell, search shift (the host entry's)
    DevBuf full_cand;                   // the search's host entries: the candidates, f32 [npeaks][N][3]
    DevBuf full_surf;                   // the search's host entries: the surfaces, f32 [N][(2R+1)^2]
    // mimc3_match_ncc_full_fb: the backward search's rows ((1 + npeaks) N of them) -- xyuvav' [rows][6], shift' [rows][2], its records
    // [rows][8], one reason byte per row -- and the host entry's fb [rows][4]
    DevBuf fb_xy, fb_sh, fb_rec, fb_why, fb_out;
    // mimc3_stack_* (stack.cpp): the stack (NCC surfaces accumulated over several pairs; state of its own, which the image setters never
    // touch) -- sum f64 [N][S^2], cnt u16 [N][S^2], lay u16 [N], shift i32 [N][2] (zeros when none was given; a host copy for the host
    // entry's bounds check); the layer scratch of an add (surfaces and records of one chunk of points) and the staging of the host
    // entries.  A weighted stack (the first add with a weight other than 1 makes it one) has wsum f64 [N][S^2] as well; lsh i32 [N][2] is
    // the layer shift of the scaled add that is under way
    struct Stack {
        DevBuf sum, cnt, lay, shift;
        DevBuf wsum, lsh;
        bool weighted = false;
        DevBuf layer, rec, ref;         // one chunk: f32 [chunk][S^2], f32 [chunk][8]; the host entry's refused flags [N]
        DevBuf out, cand, surf, count;  // mimc3_stack_finish's host entry
        std::vector<int32_t> h_shift;
        int32_t N = 0, R = 0, layers = 0;
    } stk;
};

namespace mimc3 {
// ---- capi.cpp ----
// host <-> device copies on the context's stream (pageable memory goes through two pinned chunks); d2h_copy returns with the bytes
int h2d_copy(mimc3_ctx *c, void *dst, const void *src, size_t bytes);
int d2h_copy(mimc3_ctx *c, void *dst, const void *src, size_t bytes);
// MIMC3_EBOUNDS for the first grid point g0 <= g < g1 whose chip leaves the image
int check_chips(const mimc3_ctx *c, const double *xyuvav, int32_t g0, int32_t g1, int32_t ocw, const char *entry, double *uv = nullptr);
// the MatchU8Args fields the DLC and exhaustive-search entries share: level-0 plane geometry and the grid
MatchU8Args u8_args(const mimc3_ctx *c, const double *d_xy, int32_t xy_stride, int32_t xy_col, int32_t N, int32_t off_u, int32_t off_v,
                    int32_t ocw, int32_t swap, float *d_out);
// the plane-set builders: each works on the context's stream and drains it
int build_u8_tables(mimc3_ctx *c);
int build_u16(mimc3_ctx *c, bool tables);
int build_f32(mimc3_ctx *c);

// ---- search.cpp: the host layer of the exhaustive-search family.  A public entry describes its call (SearchCall) and
//      what it accepts (SearchRules); search_check refuses, pick_kernel selects, plane_set points at the planes, launch_search launches ----
struct SearchCall {
    const char *entry;                  // the entry the caller called (for messages)
    bool host;                          // a host entry's description: the pointers are host memory, and only looked at for null
    const double *d_xyuvav;             // the points: xyuvav rows (stride 6, column 2), or a pyramid level's positions (stride 2, column 0)
    int32_t xy_stride, xy_col;
    int32_t N, off_u, off_v;
    const int32_t *d_shift;             // int32 [N][2] or null
    int32_t ocw, R, npeaks, swap;
    int32_t mode;                       // 0: the kernel of the pair's class; 1: the float kernel (what the wide entries and the stack pass)
    int32_t levels;                     // the pyramid entries' (0 elsewhere)
    float *d_out, *d_cand, *d_surf, *d_fb;
    int32_t *d_peak;                    // pyramid levels: every point's arg-max cell
    hipStream_t stream;
    // a fused stack layer (mimc3_stack_add_fused on the four run-time-ocw matrix-core kernels): the stack's planes from the call's first
    // point on -- the kernel runs its accumulating forms and writes nothing else (d_out, d_cand, d_surf null); null = an ordinary search
    double *stk_sum;
    uint16_t *stk_cnt, *stk_lay;
    double *stk_wsum;                   // a weighted stack's, or null
    // ... a SCALED one (mimc3_stack_add_scaled_fused): the stack's shift [N][2] and radius, the layer's scale and weight -- d_shift and R are
    // then the LAYER's shift and radius; stk_shift null = an unscaled layer
    const int32_t *stk_shift;
    int32_t stk_R;
    double stk_scale, stk_weight;
};
enum PairClass { kU8, kScaledInt, kIntegralF32, kFloat };             // a pair's class; an entry takes every class up to its rules' widest
enum CandRule { kCandAbsent, kCandOptional, kCandMandatory };
struct SearchRules {
    PairClass widest;
    bool has_mode;                      // takes `mode` (refused unless 0 or 1)
    bool wide;                          // the radius limit is wide_max_radius(ocw), not 15
    CandRule cand;
    bool fb = false;                    // returns forward-backward rows: d_fb is required
    bool pyramid = false;               // takes `levels`
    bool layer = false;                 // a stack's layer add: no record of its own, and a radius that the stack refuses in its own words
    bool class_surf = false;            // the surfaces come from whichever kernel runs, an integer class's too (mimc3_match_ncc_full_surf,
                                        // where they are mandatory, and the stack's class layers)
    bool any_ocw = false;               // every chip half-width 1 .. kFullChipMaxOcw, not the six alone (mimc3_match_ncc_full_chip): what
                                        // the other kernels are not built for, and all of mode 1, runs the run-time-ocw kernel
    bool chip_class = false;            // with any_ocw (mimc3_match_ncc_full_chip_class): an 8-bit pair at a chip size outside the six, and in all
                                        // of mode 1 (which takes no other class), runs the run-time-ocw matrix-core kernel; mode 0 at one of the
                                        // six is the class dispatch; whichever kernel runs serves the surfaces, which stay optional
    bool chip_planes = false;           // with chip_class (mimc3_match_ncc_full_chip_planes): a scaled-integer pair at a chip size outside the six, and
                                        // every 8-bit or scaled-integer pair in mode 1 (which takes no other class), runs the run-time-ocw
                                        // matrix-core kernel on the u16 planes
    bool wide_class = false;            // with chip_class (mimc3_match_ncc_wide_class): the radius limit is wide_u8_max_radius(ocw); beyond R 15 an
                                        // 8-bit pair runs the matrix-core wide kernel (mode 1 always, mode 0 where wide_mode0 names it or the
                                        // float wide kernel does not take the call), any other class the float wide kernel where that takes it
    bool wide_planes = false;           // with wide_class and chip_planes (mimc3_match_ncc_wide_planes): beyond R 15 a scaled-integer pair runs the
                                        // matrix-core wide kernel on the u16 planes (mode 1 always, an 8-bit pair included; mode 0 where
                                        // wide_planes_mode0 names it or the float wide kernel does not take the call), up to
                                        // wide_u16_max_radius(ocw); R <= 15 is the chip_planes entry
    bool pyramid_chip = false;          // with pyramid and any_ocw (mimc3_match_ncc_pyramid_chip): the kernel is pyramid_chip_kernel's, one of the
                                        // run-time-ocw kernels wherever the table in include/mimc3_hip.h names it, on the levels of the pair's class
    bool wide_chip = false;             // with any_ocw (mimc3_match_ncc_wide_chip): the radius limit is wide_chip_max_radius(ocw) and no pair is
                                        // refused in either mode; the kernel is wide_chip_kernel's (the table in include/mimc3_hip.h), the
                                        // run-time-ocw wide float kernel wherever no sibling takes the call; whichever kernel runs serves the surfaces
};
enum SearchKernel { Mx, U16, F32i, F32g, Wide, Chip, ChipU8, ChipU16, WideU8, WideU16, WideChip };       // last_path 6 .. 16
constexpr int kSearchKernels = 11;
// The level sets of a coarse-to-fine search: u8 planes with u8 tables, u16 planes with both tables, f32 planes reduced on their integers
// with 16-byte tables, f32 planes reduced as floats (no tables).  A pair has one integer class, so the first three share mimc3_ctx::pyr.
// level_class(kernel) is the set a kernel reads when nothing else is said; the run-time-ocw float kernel reads the integral-f32 set as
// well (its planes alone), which is why plane_set takes the class beside the kernel
enum LevelClass { kLevelU8, kLevelU16, kLevelF32i, kLevelFloat };
LevelClass level_class(SearchKernel kernel);
struct PlaneSet {
    const void *p0, *p1, *sat0, *sat1, *satz0, *satz1;
    int32_t H, W, Wp;
    double scale0, scale1;
};
bool full_ocw_ok(int32_t ocw);
// the resident pair's class; that of a pair which is neither 8-bit nor scaled-integer needs its f32 planes: built on first use (drains the stream)
int pair_class(mimc3_ctx *c, PairClass &cls);
int search_check(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules);
// host entries, after search_check: every chip inside the image, then every search box of half-width R + ocw around uv0 + offset + shift
// inside the planes' zero border (host copies; shift null = zero)
// -- or, for a pyramid entry, every starting displacement offset + shift within +-2^24, so that every level's shifts stay exact int32
int search_check_host(const mimc3_ctx *c, const char *entry, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                      int32_t ocw, int32_t R, bool pyramid = false);
int pick_kernel(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules, SearchKernel &kernel);
int plane_set(mimc3_ctx *c, SearchKernel kernel, int level, PlaneSet &planes);      // (on the levels of level_class(kernel))
int plane_set(mimc3_ctx *c, SearchKernel kernel, LevelClass levels, int level, PlaneSet &planes);
// mimc3_match_ncc_pyramid_chip's kernel for a pair class, chip size and mode (the table in include/mimc3_hip.h); false outside the table
bool pyramid_chip_kernel(PairClass cls, int32_t ocw, int32_t mode, SearchKernel &kernel);
// mimc3_match_ncc_wide_chip's kernel for a pair class, chip size, radius and mode (the table in include/mimc3_hip.h); false outside the table
bool wide_chip_kernel(PairClass cls, int32_t ocw, int32_t R, int32_t mode, SearchKernel &kernel);
int launch_search(mimc3_ctx *c, SearchKernel kernel, const PlaneSet &planes, const SearchCall &call);

// Suspends the context's timing flag for a scope: an entry made of several searches records the events around the whole call, and its
// inner launches must not move them.  The flag comes back on every way out.
struct TimingSuspended {
    mimc3_ctx *c;
    const bool was;
    explicit TimingSuspended(mimc3_ctx *ctx) : c(ctx), was(ctx->timing) { c->timing = false; }
    ~TimingSuspended() { c->timing = was; }
    TimingSuspended(const TimingSuspended &) = delete;
    TimingSuspended &operator=(const TimingSuspended &) = delete;
};
}  // namespace mimc3
