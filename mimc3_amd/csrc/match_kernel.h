// match_kernel.h -- launch interface of the matcher kernels (internal to libmimc3_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mimc3 {

constexpr int kMatchThreads = 256;   // 4 wave64 per grid point

struct MatchArgs {
    const float *i0, *i1;        // device images [H][W]
    int32_t H, W;
    const double *xyuvav;        // device [N][6]
    int32_t xy_stride, xy_col;   // the points' (u, v) sit at xyuvav[xy_stride * g + xy_col + {0, 1}]: 6, 2 (xyuvav rows) or 2, 0 (packed [N][2])
    int32_t N;
    int32_t off_u, off_v;        // CP offset, added to the search centre only (MIMC_module.c:827-828)
    const int32_t *piv_uv;       // device CSR payload [P][2]
    const int64_t *piv_off;      // device CSR offsets [N+1]
    int32_t ocw;
    int32_t swap;                // 0: chip from i0, window from i1; 1: exchanged
    int32_t win_half;            // 0: DLC window (|last pivot|+ocw+2, last row/column empty, :863-886); >0: the search area is
                                 // the full (2*win_half+1)^2 square (get_offset_image's image chips, :347)
    float thr;                   // smallest f32 whose f64 value is >= MIN_DN (1e-10, MIMC_module.c:21)
    float *out;                  // device [N][3]
    const int32_t *point_list;   // optional: process only these point indices (device list) ...
    const int32_t *point_count;  // ... whose length is read on the device (nullptr = all N points)
    // LDS carve (floats / pivots), filled by the launcher from the per-launch maxima
    int32_t lds_chip_f, lds_win_f, lds_cell_f, lds_npiv;
    // global workspace for the compact cell grid when it outgrows LDS (long diagonal corridors): kCellGlobalGrid slices
    unsigned char *cell_ws;
    size_t cell_ws_bytes, cell_ws_stride;
    int32_t cell_ws_cells;
};
constexpr int kCellGlobalGrid = 1024;   // persistent workgroups of the workspace mode (4 per CU)
size_t match_f32_workspace_bytes(int ocw, int max_abs_u, int max_abs_v, int max_npiv, int win_half);

// ---- exact-integer path for 8-bit imagery (match_u8_kernel.hip) -------------------------------
constexpr uint8_t kMxNulls = 2, kMxRest = 1, kMxWn = 3;
constexpr int kU8Pad = 256;      // zero border (pixels) around the u8 planes; multiple of 4

struct MatchU8Args {                // arguments of the register-tiled kernel family (match_px_kernel.hip)
    const unsigned char *p0, *p1;   // zero-bordered planes of i0, i1 (u8 or f32 pixels): pixel (u,v) at [(v+pad)*Wp + u+pad]
    int32_t Wp, pad;                // plane pitch (PIXELS; a whole number of dwords) and border
    float thr;                      // smallest f32 whose f64 value is >= MIN_DN (f32 policy)
    // u16 policy: plane k stores value * 2^s_k; scale_k = 2^-s_k (1.0 otherwise).  (The accumulating forms of the run-time-ocw
    // matrix-core searches, which read no plane scale: a SCALED layer's scale and weight, stack_acc.h)
    union { double scale0; double stk_scale; };
    union { double scale1; double stk_weight; };
    int32_t H, W;
    const double *xyuvav;
    int32_t xy_stride, xy_col;      // see MatchArgs
    int32_t N;
    int32_t off_u, off_v;
    // (exhaustive search, launch_match_full_mx: cells s in [-full_R, full_R]^2 around uv0 + offset + full_shift[g], out [N][8]; its two
    //  arguments share the slots of the DLC's pivots and search-area half-width, which it does not read)
    union {
        const int32_t *piv_uv;
        const int32_t *full_shift;  // per-point int32 [N][2] (u, v), or null (zero)
    };
    union {
        const int64_t *piv_off;
        int32_t *full_peak;         // exhaustive search, optional: per point the arg-max cell k, or -1 without one (pyramid levels)
    };
    int32_t ocw, swap;
    union {
        int32_t win_half;           // 0: DLC window (|last pivot|+ocw+2, last row/column empty); > 0: full (2*win_half+1)^2 search area (CP stage)
        int32_t full_R;             // exhaustive search: 1..15
    };
    float *out;
    // (exhaustive search with candidates, mimc3_match_ncc_full_multi: the best full_npeaks local maxima of every point's surface, pass-major;
    //  the pointer and the count share the slots of the overflow list and the climb's look-ahead, which full mode never reads)
    union {
        int32_t *ovf_list;          // points whose NCC cache overflowed: handed to the general kernel (list mode)
        float *full_cand;           // exhaustive search, optional: f32 [full_npeaks][N][3] (du, dv, ncc); null = the record alone
    };
    // (exhaustive search with surfaces, mimc3_match_ncc_full_surf: the surface-storing forms of the three integer-class kernels; the
    //  pointer shares the slot of the overflow list's counter, which full mode never reads)
    union {
        int32_t *ovf_count;
        float *full_surf;           // exhaustive search, optional: f32 [N][(2 full_R + 1)^2], every point's surface in k order; null = none
    };
    // list mode: workgroup b handles point_list[b], b < *point_count (nullptr = all N points).
    // (The accumulating forms of the run-time-ocw matrix-core searches, stack_acc.h: the stack's planes from the launch's first point on --
    //  sum f64 [N][S^2], cnt u16 [N][S^2], lay u16 [N], wsum f64 [N][S^2] or null.  Those kernels have neither list mode nor a fail or
    //  rest list, so the four pointers share these slots; the launchers read them only when `forms` asks for the accumulating forms)
    union { const int32_t *point_list; double *stk_sum; };
    union { const int32_t *point_count; uint16_t *stk_cnt; };
    // PxU8o: points whose chip or window does not fit a local 8-bit range.  Matrix-core DLC kernel behind u8_classify: the rest list --
    // a point the kernel meets but does not take (a climb that leaves the tile or outlasts the recorded scans: a few dozen per launch)
    // is appended with one atomicAdd, and the register-tiled kernel runs over that list right behind
    union { int32_t *fail_list; int32_t *rest_list; uint16_t *stk_lay; };
    union { int32_t *fail_count; int32_t *rest_count; double *stk_wsum; };
    // matrix-core kernel (match_mx_kernel.hip): one class byte per grid point -- 0 = its clean form takes the point, kMxWn / kMxNulls =
    // its window-null / general form does, kMxRest = none does.  The DLC path gets every byte from u8_classify (u8_classify_kernel.hip)
    // before the first launch; the exhaustive search zeroes them and lets the clean form classify (plain stores: a shared list counter
    // serialises ~100,000 same-address atomics per launch, measured 1.0 ms)
    uint8_t *mx_flags;
    int32_t mx_classified;          // DLC path: mx_flags and the point lists come from u8_classify; the clean form runs over point_list and appends what it hands on to rest_list
    int32_t mx_gen_on, mx_wn_on;    // which of its forms for null-ridden points run behind the clean form (general / window nulls only); the others' points get kMxRest
    // flag mode of every kernel of the family: workgroup b handles point b only if point_flags[b] == flag_value
    const uint8_t *point_flags;
    int32_t flag_value;
    // LDS carve, filled by the launcher
    int32_t lds_pw, lds_off_val, lds_off_vis, lds_off_list, lds_off_sums, lds_off_piv, lds_list_cap;
    int32_t lds_off_chip, lds_off_lw, lds_off_lc;   // big-chip integer configs: LDS chip copy, window-null and chip-null lists
    int32_t lds_off_traj;                           // many-pivot configs: recorded climbs of the pivots beyond the first 64
    int32_t lds_off_vals, lds_nslot;                // compact configs: value slots of the two-level NCC cache
    // PxU8o: min | max << 16 of the non-null pixels of every 16x16-pixel tile of the two u16 planes (plane coordinates), or null.
    // The 8-bit pair behind u8_classify (whose kernels read no range tiles): the point records (U8PointRec below), or null = none --
    // point_recs[i] is the header of point_list[i]; rest_recs is the array parallel to rest_list, where the matrix-core kernel puts the
    // record of a point it appends (both writable: u8_classify fills them).  ALIASED SLOTS: a caller sets either the range tiles (PxU8o,
    // the only policy that reads rt0 / rt1) or the records (the PxU8 launches behind u8_classify), never both, and clears them before
    // the argument block goes to a kernel of the other kind -- a non-null rt0 in a PxU8 launch is a record pointer
    // (The accumulating forms of the run-time-ocw matrix-core searches, which read neither: stk_shift, the STACK's shift [N][2] of a scaled
    //  layer -- full_shift is then the layer shift -- or null = an unscaled layer, and stk_R, the stack's radius)
    union { const uint32_t *rt0; struct U8PointRec *point_recs; const int32_t *stk_shift; };
    union { const uint32_t *rt1; struct U8PointRec *rest_recs; };
    union { int32_t rt_tw; int32_t stk_R; };        // tiles per plane row
    int32_t replay_shortcut;                        // DLC kernels: the exact replay tries the winning pivot alone first (replay_shortcut_on;
                                                    // filled by the launchers; in the four bytes the table pointers' alignment left unused)
    // packed summed-area tables of the two planes (sat_kernel.hip; policies with P::SAT), (Hp + 1) rows of sat_ws entries
    const void *sat0, *sat1;
    const void *satz0, *satz1;      // u16 planes: null counts (u32), same geometry
    int32_t sat_ws;
    union {
        int32_t lookahead;          // speculative climb: 3x3 blocks requested ahead along a straight move
        int32_t full_npeaks;        // exhaustive search with candidates: 1..8
    };
    unsigned long long *stats;     // diagnostics only (env MIMC3_U8_STATS): per-phase s_memtime sums
    int32_t debug_stop;             // diagnostics only (env MIMC3_U8_DEBUG_STOP): leave the kernel after phase k; 0 = off
    int32_t dry_run;                // launcher only: compute the LDS carve and return hipSuccess / hipErrorInvalidValue (does not fit
                                    // 160 KB) without launching -- the C ABI asks this before it commits to a kernel policy
};

// What u8_classify has read and derived of a point to class it, kept for the two matcher kernels: one record per list position, so that
// a workgroup's header is ONE load behind the list length (16 lanes, a dword each, fields by readlane) instead of the chain list entry ->
// point row and pivot range -> last pivot -> table queries.  Everything in it is independent of the kernels' template parameters.
struct alignas(64) U8PointRec {
    int32_t g;                      // the point
    int32_t u0, v0;                 // its chip centre (image pixels)
    int32_t lu, lv;                 // its last pivot
    int32_t npiv;                   // bits 0-7 (behind u8_classify no call has more than 64 pivots per point) | the climb area << 8 (mx_area_pack)
    int64_t pbeg;                   // piv_off[g]
    uint32_t tile;                  // tx0 | ty0 << 10 | fits << 20 (mx_tile_fit of the DLC tile, origin 1) | done << 21 (kRecDone) | the chip's corner pixel << 24 (clean and advance points)
    int32_t win_nulls;              // nulls of the window's written area
    unsigned long long chipQ;       // the chip's packed table query (sum, sum of squares, nulls)
    unsigned long long colQ, rowQ;  // clean points only: the queries of the chip's last column and last row (the matrix-core kernel's closed-form T4 terms)
};
static_assert(sizeof(U8PointRec) == 64, "U8PointRec: one 64-byte line, sixteen dwords");

// ---- what the matrix-core DLC kernel takes: shared by its header and by u8_classify, so that the two cannot drift apart ----------
// The 32 x 32 cell tile of a point whose last pivot is (lu, lv) and whose compact cell grid is csx x csy (a climb touches [1, cs - 2]):
// all reachable cells if they fit (origin tile0), else centred on the pivots' starts; false = the pivot set is wider than the tile
__device__ __forceinline__ bool mx_tile_fit(int lu, int lv, int ocw, int dx2, int dy2, int csx, int csy, int tile0, int &tx0, int &ty0)
{
    tx0 = tile0; ty0 = tile0;
    bool fits = true;
    const int c0x = dx2 - ocw, c1x = c0x + lu, c0y = dy2 - ocw, c1y = c0y + lv;
    const int lox = min(c0x, c1x), hix = max(c0x, c1x), loy = min(c0y, c1y), hiy = max(c0y, c1y);
    if (csx - 2 > 32) { tx0 = min(max((lox + hix) / 2 - 15, 1), csx - 2 - 31); fits = fits && lox - 1 >= tx0 && hix + 1 <= tx0 + 31; }
    if (csy - 2 > 32) { ty0 = min(max((loy + hiy) / 2 - 15, 1), csy - 2 - 31); fits = fits && loy - 1 >= ty0 && hiy + 1 <= ty0 + 31; }
    return fits;
}
// The climb area of a point: the rectangle of cells spanned by pivot 0's cell and the last pivot's, grown by kMxAreaGrow cells on every
// side, clipped to the reachable cells [1, cs - 2] and to the tile (tx0, ty0 of mx_tile_fit).  DLC pivots run from (0, 0) to the last
// pivot, so their climbs rarely leave it.  a[] = its bounds as tile-relative cells (x0, x1, y0, y1, inclusive, each 0..31); (px, py, pw, ph)
// = the union of those cells' boxes in window pixels, clipped to the window's written area (2 dx2 x 2 dy2: the never-written last row and
// column are not window pixels, the clean form's closed-form T4 terms stand for them).  If that rectangle holds no null, n, sx and sxx of
// every cell of the area are what they are for a null-free window, and the matrix-core kernel's clean form computes those cells exactly
// -- whatever nulls the rest of the window holds: a climb whose every scan stays inside the area never reads another cell.
constexpr int kMxAreaGrow = 2;
__device__ __forceinline__ void mx_climb_area(int lu, int lv, int ocw, int dx2, int dy2, int csx, int csy, int tx0, int ty0, int (&a)[4], int &px,
                                              int &py, int &pw, int &ph)
{
    const int c0x = dx2 - ocw, c1x = c0x + lu, c0y = dy2 - ocw, c1y = c0y + lv;
    const int lox = max(max(min(c0x, c1x) - kMxAreaGrow, 1), tx0), hix = min(min(max(c0x, c1x) + kMxAreaGrow, csx - 2), tx0 + 31);
    const int loy = max(max(min(c0y, c1y) - kMxAreaGrow, 1), ty0), hiy = min(min(max(c0y, c1y) + kMxAreaGrow, csy - 2), ty0 + 31);
    a[0] = lox - tx0; a[1] = hix - tx0; a[2] = loy - ty0; a[3] = hiy - ty0;
    px = lox; py = loy;                                         // (the box of cell c: window pixels c .. c + 2 ocw)
    pw = min(hix + 2 * ocw + 1, 2 * dx2) - lox; ph = min(hiy + 2 * ocw + 1, 2 * dy2) - loy;
}
// the area's bounds in a record (U8PointRec::npiv, bits 8-27), and the whole tile: what a point carries when areas are off (mx_area_on).
// The clean form finishes the NCC of the area's cells alone (whole bands of four tile rows), so a clean point carries its area as well
__device__ __forceinline__ uint32_t mx_area_pack(const int (&a)[4]) { return ((uint32_t)a[0] | (uint32_t)a[1] << 5 | (uint32_t)a[2] << 10 | (uint32_t)a[3] << 15) << 8; }
constexpr uint32_t kMxAreaTile = (0u | 31u << 5 | 0u << 10 | 31u << 15) << 8;
constexpr uint32_t kRecNpivMask = 0xffu;
constexpr uint32_t kRecDone = 1u << 21;     // U8PointRec::tile of a rest-list record: the matrix-core launch has finished the point (advance list)
// A scan centred on tile-relative cell (rx, ry) reads nine cells.  It is allowed when all nine lie inside the area, i.e. when
// (unsigned)(rx - xlo) <= wx && (unsigned)(ry - ylo) <= wy with the four numbers below (an area too narrow for any scan: none passes).
// The whole tile gives 1, 29, 1, 29
__device__ __forceinline__ void mx_area_scan_bounds(uint32_t rec_npiv, int &xlo, uint32_t &wx, int &ylo, uint32_t &wy)
{
    const uint32_t area = rec_npiv >> 8;
    const int x0 = (int)(area & 31u), x1 = (int)((area >> 5) & 31u), y0 = (int)((area >> 10) & 31u), y1 = (int)((area >> 15) & 31u);
    const bool some = x1 - x0 >= 2 && y1 - y0 >= 2;
    xlo = some ? x0 + 1 : 64; wx = some ? (uint32_t)(x1 - x0 - 2) : 0u;
    ylo = some ? y0 + 1 : 64; wy = some ? (uint32_t)(y1 - y0 - 2) : 0u;
}
// no form of the kernel takes a point with more pivots than a wave has lanes (or none) or a pivot set wider than the tile
__device__ __forceinline__ bool mx_takes(int npiv, bool fits) { return npiv >= 1 && npiv <= 64 && fits; }
// the class of a point the kernel could take, from the null counts of the window's written area and of the chip (0 = the clean form's)
__device__ __forceinline__ uint8_t mx_null_class(int win_nulls, int chip_nulls, int wn_on, int gen_on)
{
    if (win_nulls == 0 && chip_nulls == 0) return 0;
    return (chip_nulls == 0 && wn_on) ? kMxWn : (gen_on ? kMxNulls : kMxRest);
}

// f32 image -> zero-bordered u8 plane (plane must be pre-zeroed); *d_flag is set to 1 if any pixel
// is not an integer in [0,255] (then the u8 path must not be used for this image).
hipError_t launch_prep_u8(const float *img, int H, int W, unsigned char *plane, int Wp, int pad, int *d_flag, hipStream_t s);
// raw DN as the TIFF holds it -> f32 image (+ the u8 plane for 8-bit DN; plane pre-zeroed): the widening of
// GMA_float_load_tiff (GMA.c:288-310) done on the device so that only the raw bytes cross PCIe
hipError_t launch_widen_u8(const unsigned char *raw, int H, int W, float *img, unsigned char *plane, int Wp, int pad, hipStream_t s);
hipError_t launch_widen_u16(const unsigned short *raw, size_t n, float *img, hipStream_t s);
// instantiated chip sizes and border reach (|last pivot| + |CP offset| must fit in the border)
bool match_u8_supported(int ocw, int max_reach_u, int max_reach_v);
// same kernel family on zero-bordered u16 planes of scaled integers (q = value * 2^shift < 4096): same chip sizes as u8
hipError_t launch_detect_scaled_int(const float *img, size_t n, int *d_flags, hipStream_t s);
hipError_t launch_prep_u16(const float *img, int H, int W, unsigned short *plane, int Wp, int pad, int shift, hipStream_t s);
hipError_t launch_match_u16(MatchU8Args a, int max_abs_u, int max_abs_v, int max_npiv, hipStream_t stream);
// u16 planes of INTEGERS read through a per-point offset into the u8 kernels (points that do not fit go to fail_list)
hipError_t launch_match_u8o(MatchU8Args a, int max_abs_u, int max_abs_v, int max_npiv, hipStream_t stream);
// fraction-of-tiles estimate for the above: out[0] += tiles whose non-null range fits 8 bits, out[1] += tiles with data
hipError_t launch_range_tiles(const unsigned short *plane, int H, int W, int Wp, int pad, int *d_out2, hipStream_t s);
// tiles [ceil(Hp/16)][ceil(Wp/16)] of a zero-bordered u16 plane (Hp rows): min | max << 16 over the non-null pixels (0xffff | 0 if none)
hipError_t launch_range_tiles16(const unsigned short *plane, int Hp, int Wp, uint32_t *tiles, hipStream_t s);
// same kernel family on zero-bordered f32 planes (any f32 imagery; small chips only)
hipError_t launch_prep_f32(const float *img, int H, int W, float *plane, int Wp, int pad, hipStream_t s);
bool match_f32x_supported(int ocw, int max_reach_u, int max_reach_v);
hipError_t launch_match_f32x(MatchU8Args a, int max_abs_u, int max_abs_v, int max_npiv, hipStream_t stream);
hipError_t launch_match_u8(MatchU8Args a, int max_abs_u, int max_abs_v, int max_npiv, hipStream_t stream);
// dense correlation surfaces on the matrix cores (8-bit planes with tables; match_mx_kernel.hip): takes the points whose cell grid
// fits its tile and whose chip and window have no null.  u8_classify runs first (one thread per point, once per call): it writes every
// point's class byte and the two index lists in ascending point order -- `lists`: [0] clean count, [1] rest count, [2] advance count,
// [kU8ListHead, + N) the clean list, then N words of rest list, N words of advance list (rest-list POSITIONS of the window-null points whose
// climb area is null-free, mx_climb_area above: the clean form tries them in the same launch and marks those it finishes in their rest
// records) and u8_classify_scratch_ints(N) of scratch -- and zeroes a.ovf_count.  The clean form then runs over the clean list and
// appends what it hands on to the rest list, which is launch_match_u8's in list mode right behind.
bool match_mx_supported(int ocw, int max_npiv, int win_half, int max_abs_u, int max_abs_v);
constexpr int kU8ListHead = 4;
size_t u8_classify_scratch_ints(int N);
// ... and with point records (U8PointRec): the bytes of `lists` with the records behind the scratch, and where they start -- [N] parallel
// to the clean list, [N] parallel to the rest list, [N] of the classifier's staging.  launch_match_mx sets them up in its own launches when
// u8_point_records_on(); the caller hands the rest records (u8_list_recs(lists, N) + N) to launch_match_u8 with the rest list
size_t u8_lists_bytes(int N);
U8PointRec *u8_list_recs(int32_t *lists, int N);
bool u8_point_records_on();        // (tuning / A-B: MIMC3_U8_RECS=0 keeps the memory headers)
bool u8_advance_on();              // (tuning / A-B: MIMC3_U8_ADVANCE=0, or no records, leaves the advance list empty)
bool mx_area_on();                 // (tuning / A-B: MIMC3_MX_AREA=0, or no advance list, gives clean points the whole tile as their area)
bool mx_box_table_on();            // (tuning / A-B: MIMC3_MX_BOX_TABLE=0 gives the record forms the MFMA box sums back; else they read the window plane's table)
// The exact replay of both DLC kernels first replays the winning pivot alone (match_mx_kernel.hip, "the shortcut"; match_px_kernel.hip's
// fast register form); tests / A-B: MIMC3_REPLAY_SHORTCUT=0 forces the full replay.  What a point did, as the diagnostics count it
// (MIMC3_MX_STATS, MIMC3_U8_STATS):
bool replay_shortcut_on();
constexpr uint32_t kReplayShort = 0u, kReplayShortU = 1u, kReplayFellBack = 2u, kReplayNoPre = 3u;   // taken with U empty / with U built, fell back, preconditions failed
hipError_t launch_match_mx(MatchU8Args a, int32_t *lists, hipStream_t stream);
// (u8_classify_kernel.hip; wn_on / gen_on: which forms for null-ridden points run behind the clean form)
// advance: also write the advance list (needs the records) -- else its length is 0; clean_area: clean points' records carry their
// climb area (mx_climb_area) instead of the whole tile
hipError_t launch_u8_classify(const MatchU8Args &a, int32_t *lists, bool advance, bool clean_area, hipStream_t stream);
// exhaustive-search NCC offsets on the same surfaces (mimc3_match_ncc_full): every point on the matrix cores -- the clean form, then
// the window-null and general forms over the points it flags (a.mx_flags: N bytes, zero before the call); a.full_R in 1..15,
// a.ocw one of 7, 15, 16, 30, 32, 40; a.out [N][8]; a.full_peak (optional, int32 [N]) gets every point's arg-max cell k = (su + R)(2R + 1)
// + (sv + R), also at status -4, or -1 without one (status -3 / -2, the NaN record of a point outside the image or the zero border);
// a.full_cand (optional, f32 [a.full_npeaks][N][3], 1 <= full_npeaks <= kFullMaxPeaks; not together with full_peak) gets every point's
// best local maxima as (du, dv, ncc) candidates (mimc3_match_ncc_full_multi) -- null selects the kernels without that tail;
// a.full_surf (optional, f32 [N][(2 full_R + 1)^2]; not together with full_peak) gets every point's surface in k order, k = (su + R)(2R + 1)
// + (sv + R), from the form that finishes the point -- all NaN where the record is all NaN or has status -3 -- and selects the SURF forms
constexpr int kFullMaxPeaks = 8;
hipError_t launch_match_full_mx(MatchU8Args a, hipStream_t stream);
// the same search on the zero-bordered u16 planes of a scaled-integer pair (match_full_u16_kernel.hip): a.p0 / a.p1 the u16 planes, a.sat0 /
// a.sat1 their packed tables, a.satz0 / a.satz1 their null tables; a.full_shift, a.full_R, a.full_peak, a.full_cand / a.full_npeaks and a.out as
// above, a.full_surf too.  Two launches, the points without nulls and those with; no flags, lists or scratch
hipError_t launch_match_full_u16(MatchU8Args a, hipStream_t stream);
// the same search on the zero-bordered f32 planes of an integral-f32 pair (match_full_f32_kernel.hip; 16-bit DN and its filtered forms):
// a.p0 / a.p1 the f32 planes, a.sat0 / a.sat1 their 16-byte tables (Sat2), a.scale0 / a.scale1 = 2^-s of each image (pixel * 2^s is the
// integer the tables sum); the rest as above.  Two launches, dynamic LDS sized by a.full_R
hipError_t launch_match_full_f32(MatchU8Args a, hipStream_t stream);
// the same search on the zero-bordered f32 planes of ANY f32 pair (match_full_f32g_kernel.hip; non-integral pixels, NaN and negative
// nulls): a.p0 / a.p1 the f32 planes, no tables; surf (optional, f32 [N][(2R+1)^2]) gets every point's surface in k order; a.full_peak
// (optional; not together with full_cand or surf) the arg-max cells, summed in the order of the record-only form.  One launch
hipError_t launch_match_full_f32g(MatchU8Args a, float *surf, hipStream_t stream);
// the same search over a range of up to +-47 px (match_wide_kernel.hip; mimc3_match_ncc_wide): the arguments of launch_match_full_f32g
// without a.full_peak, a.full_R in 1 .. wide_max_radius(a.ocw) -- the largest radius whose box, chip and surface fit a CU's LDS at this
// chip size (0 for an ocw the kernel is not built for), from the constexpr layout the launch uses.  One launch, dynamic LDS sized by a.full_R
int wide_max_radius(int ocw);
int wide_lds_bytes(int ocw, int R);     // the dynamic LDS of a launch at radius R (0 outside 1 .. wide_max_radius(ocw))
hipError_t launch_match_wide(MatchU8Args a, float *surf, hipStream_t stream);
// the same search at ANY chip half-width 1 <= a.ocw <= kFullChipMaxOcw (match_full_chip_kernel.hip; mimc3_match_ncc_full_chip): the arguments
// of launch_match_full_f32g, a.full_peak included (not together with full_cand or surf); a.ocw is a run-time value, the chip is walked in bands of full_chip_band_rows(ocw, R) chip
// rows (the whole chip where it fits), each band within kChipLdsBudget bytes of dynamic LDS.  One launch
constexpr int kFullChipMaxOcw = 80;
constexpr int kChipLdsBudget = 79 * 1024;       // two workgroups per CU (160 KB), their static slots included
int full_chip_band_rows(int ocw, int R);        // 0 outside 1 <= ocw <= kFullChipMaxOcw, 1 <= R <= 15
hipError_t launch_match_full_chip(MatchU8Args a, float *surf, hipStream_t stream);
// the same search at any chip half-width on the u8 planes of an 8-BIT pair, on the matrix cores (match_full_chip_u8_kernel.hip;
// mimc3_match_ncc_full_chip_class): a.p0 / a.p1 the u8 planes, a.sat0 / a.sat1 their packed tables, a.mx_flags N class bytes, zero before
// the call; a.full_shift, a.full_R, a.full_cand / a.full_npeaks, a.full_surf and a.out as launch_match_full_mx takes them; a.full_peak
// (optional; not together with full_cand, full_surf or the accumulating forms) selects the PEAK forms: every point gets exactly one store,
// its arg-max cell or -1, from the form that finishes it -- the clean form also for the NaN record, the masked form for its -3.
// forms: bit 0 the clean form over all points (it flags the points that hold a null), bit 1 the masked form over the flagged points --
// 3 is the search, 1 and 2 are for timing the forms apart.  Bit 2 (kFormsAcc, with any of the above; this kernel and the three below)
// selects the ACCUMULATING forms (stack_acc.h): each point's finished surface is added into the stack at a.stk_sum / a.stk_cnt / a.stk_lay
// (/ a.stk_wsum) in the tail's place -- no record, candidate or surface is written, so a.out, a.full_cand and a.full_surf must be null.
// With a.stk_shift set the layer is a SCALED one (mimc3_stack_add_scaled_fused): a.full_R and a.full_shift are the layer's, a.stk_R (1 ..
// kStackAccMaxRadius) and a.stk_shift the stack's, a.stk_scale and a.stk_weight the layer's scale and weight, and every workgroup
// resamples its point's surface onto the stack's cells (stack_acc_scaled); a.stk_shift null is the unscaled layer, as before.
// full_chip_u8_layout: K chunks per chip row, 16-row tiles and K chunks of the
// box sums, dynamic LDS bytes of a launch at this ocw (false outside 1 .. kFullChipMaxOcw)
constexpr int kFormsAcc = 4;
constexpr int kStackAccMaxRadius = 47;  // (stack_kernel.h's kStackMaxRadius: stack_kernel.hip asserts the two equal)
bool full_chip_u8_layout(int ocw, int out[4]);
hipError_t launch_match_full_chip_u8(MatchU8Args a, int forms, hipStream_t stream);
// ... and on the u16 planes of a SCALED-INTEGER pair (q < 4096; match_full_chip_u16_kernel.hip; mimc3_match_ncc_full_chip_planes): a.p0 / a.p1
// the u16 planes, a.sat0 / a.sat1 their packed tables, a.satz0 / a.satz1 their null tables, the rest as above (forms included)
bool full_chip_u16_layout(int ocw, int out[4]);
hipError_t launch_match_full_chip_u16(MatchU8Args a, int forms, hipStream_t stream);
// the search beyond +-15 px on the u8 planes of an 8-BIT pair at any chip half-width, on the matrix cores (match_wide_u8_kernel.hip;
// mimc3_match_ncc_wide_class): the arguments and forms of launch_match_full_chip_u8 (no PEAK forms: no a.full_peak) with 16 <= a.full_R <= 47 -- that kernel over a grid of
// 32 x 32 cell tiles, the surface at pitch 96 in LDS bytes of its own, the tails of match_full_tail.h and match_wide_tail.h.
// wide_u8_max_radius: 47 for 1 <= ocw <= kFullChipMaxOcw, else 0.  wide_u8_layout_query: K chunks per chip row, cell tiles per axis, threads
// per workgroup, dynamic LDS bytes of a launch at (ocw, R) (false outside 1 .. kFullChipMaxOcw x 16 .. 47), from the constexpr layout the launch uses
int wide_u8_max_radius(int ocw);
bool wide_u8_layout_query(int ocw, int R, int out[4]);
hipError_t launch_match_wide_u8(MatchU8Args a, int forms, hipStream_t stream);
// ... and on the u16 planes of a SCALED-INTEGER pair (q < 4096; match_wide_u16_kernel.hip; mimc3_match_ncc_wide_planes): the arguments and
// forms of launch_match_full_chip_u16 with 16 <= a.full_R <= wide_u16_max_radius(a.ocw) -- that kernel over the same grid of 32 x 32 cell
// tiles.  wide_u16_max_radius: the largest R <= 47 whose two tiles, two chip planes and surface fit a CU's LDS (47 up to ocw 68, 27 at
// ocw 80; 0 outside 1 .. kFullChipMaxOcw).  wide_u16_layout_query: as wide_u8_layout_query (false outside 16 .. wide_u16_max_radius(ocw))
int wide_u16_max_radius(int ocw);
bool wide_u16_layout_query(int ocw, int R, int out[4]);
hipError_t launch_match_wide_u16(MatchU8Args a, int forms, hipStream_t stream);
// the search beyond +-15 px on the f32 planes of ANY pair at any chip half-width (match_wide_chip_kernel.hip; mimc3_match_ncc_wide_chip): the
// arguments of launch_match_wide with 1 <= a.ocw <= kFullChipMaxOcw and 16 <= a.full_R <= 47 -- launch_match_full_chip's band loop once per
// 32 x 32 cell tile, the surface at pitch 96 in LDS bytes of its own.  wide_chip_max_radius: 47 for 1 <= ocw <= kFullChipMaxOcw, else 0.
// wide_chip_layout_query: cell tiles per axis, chip rows per band, bands, workgroups per CU the LDS allows, dynamic LDS bytes of a launch
// at (ocw, R) (false outside 1 .. kFullChipMaxOcw x 16 .. 47), from the constexpr layout the launch uses
int wide_chip_max_radius(int ocw);
bool wide_chip_layout_query(int ocw, int R, int out[5]);
hipError_t launch_match_wide_chip(MatchU8Args a, float *surf, hipStream_t stream);
static_assert(sizeof(MatchU8Args) == 344,"MatchU8Args: the unions over its slots keep the struct's size");
// The coarse-to-fine search (mimc3_match_ncc_pyramid, pyramid_kernel.hip).  One level of a zero-bordered u8 plane pair from the level
// above: pixel (x, y) = the rounded mean (s + n/2) / n of the non-zero pixels of the 2 x 2 block at (2x, 2y), 0 if the block is all
// zero; Hd = Hs >> 1, Wd = Ws >> 1 (the destination plane pre-zeroed, border pad in both)
hipError_t launch_pyr_reduce(const unsigned char *src, int Hs, int Ws, int Wps, unsigned char *dst, int Hd, int Wd, int Wpd, int pad,
                             hipStream_t s);
// The same rule on the integers the other two plane types stand for (mimc3_match_ncc_pyramid_dn): a u16 plane's values q = pixel * 2^s,
// and an f32 plane's w = pixel * 2^shift (an integer below 2^20; the level pixel is the reduced integer times 2^-shift).  The level
// inherits the image's shift
hipError_t launch_pyr_reduce_u16(const unsigned short *src, int Hs, int Ws, int Wps, unsigned short *dst, int Hd, int Wd, int Wpd, int pad,
                                 hipStream_t s);
hipError_t launch_pyr_reduce_f32(const float *src, int Hs, int Ws, int Wps, float *dst, int Hd, int Wd, int Wpd, int pad, int shift,
                                 hipStream_t s);
// ... and on the f32 plane of any float pair (mimc3_match_ncc_pyramid_any): the f64 mean, rounded to f32, of the block's pixels with
// (double)p >= 1e-10 added in row-major order, 0 when there is none; no shift, and no tables are built for these levels
hipError_t launch_pyr_reduce_f32g(const float *src, int Hs, int Ws, int Wps, float *dst, int Hd, int Wd, int Wpd, int pad, hipStream_t s);
// Per point before the search of level `lnext`: its starting displacement D = (off_u, off_v) + shift[g] (shift null = 0) scaled to the
// coarsest level (first: d = floor((D + 2^(L-2)) / 2^(L-1)), L = lnext + 1), or the step d = 2 (d_l + s) / 2 d_l from the level just
// searched (d_l = sh[g], s its arg-max peak[g]); writes sh[g] = d, or d - (off_u, off_v) when lnext == 0, and the level's
// grid-point position pos[g] = (u0 >> lnext, v0 >> lnext) (f64, lnext > 0)
hipError_t launch_pyr_step(const double *xyuvav, int N, int off_u, int off_v, const int32_t *shift, const int32_t *peak, int R, int lnext,
                           bool first, int32_t *sh, double *pos, hipStream_t s);

// max_abs_u/v: max over points of |last pivot| per axis; max_npiv: max pivots per point.
hipError_t launch_match_f32(MatchArgs a, int max_abs_u, int max_abs_v, int max_npiv, hipStream_t stream);

}  // namespace mimc3
