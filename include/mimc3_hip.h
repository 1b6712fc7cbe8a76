/*
 * mimc3_hip.h -- C ABI of libmimc3_hip.so: the MI355X (gfx950) implementation of MIMC3's
 * per-grid-point DLC/NCC matching loop and QM pseudo-smoothing update.
 *
 * The reference has no plugin/FFI layer; its seam for this path is three plain C functions
 * (MIMC_module.h:41,46,58).  Each entry point below names the reference interface it replaces.
 * Plain pointers and sizes only; no GMA structs here (see mimc3_gma_shim.h for the struct-level
 * drop-in with the reference's exact signatures), no torch types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative MIMC3_E* code, or a positive hipError_t;
 *     mimc3_last_error() returns a thread-local message for the last failure.
 *   - images are row-major float32 [H][W] as produced by GMA_float_load_tiff (GMA.c:246-316).
 *   - xyuvav is row-major float64 [N][6] = map x, map y, image u, image v, a-priori vx, vy.
 *   - DLC pivots are CSR: piv_off int64 [N+1], piv_uv int32 [P][2] (u, v offsets), which is the
 *     flattening of the reference's ragged `GMA_int32 **uv_pivot`.
 *   - "_dev" functions take DEVICE pointers and enqueue on the given hipStream_t (passed as
 *     void*; NULL = the default stream) without synchronising; the others take HOST pointers,
 *     copy, run, and synchronise (drop-in semantics).
 *   - a context owns scratch that its calls share (overflow lists, planes, staging buffers): keep ONE stream in flight
 *     per context -- issue the "_dev" calls of a context on one stream, and drain it before a call that rebuilds the
 *     planes (set_images*, filter_images).  Concurrency comes from several contexts (one per device, or several per
 *     device: the control-point stage does exactly that internally).
 *   - there is NO CPU fallback anywhere in this library.
 */
#ifndef MIMC3_HIP_H
#define MIMC3_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MIMC3_EINVAL   (-1)  /* bad argument (null pointer, non-positive size, ocw < 2 ...)      */
#define MIMC3_EBOUNDS  (-2)  /* a chip would leave the image, or a point has zero pivots: the
                                reference reads/writes out of bounds there (MIMC_module.c:852,
                                :589-591); this library refuses instead                        */
#define MIMC3_ECAP     (-3)  /* caller-provided output capacity too small                        */
#define MIMC3_ENODEV   (-4)  /* no usable HIP device                                             */
#define MIMC3_ESTATE   (-5)  /* context in the wrong state (e.g. images not set)                 */
#define MIMC3_EUNSUPPORTED (-6)  /* input kind the entry point does not handle (yet), e.g. a pair that
                                is not 8-bit for mimc3_match_ncc_full                             */

typedef struct mimc3_ctx mimc3_ctx;   /* opaque: device id, stream, resident images, workspaces */

/* ---- context: keeps both images resident in HBM across the CLI's 32 matcher passes
 *      (MIMC_main.c:261-350 calls the matcher 32x on 4 image pairs) ------------------------- */
int  mimc3_ctx_create(int device, mimc3_ctx **out);
void mimc3_ctx_destroy(mimc3_ctx *ctx);
const char *mimc3_last_error(void);

/* Upload a host image pair (replaces the reference holding GMA_float *i0,*i1 in host RAM). */
int mimc3_ctx_set_images(mimc3_ctx *ctx, const float *i0, const float *i1, int32_t H, int32_t W);
/* The same from the RAW DN the TIFF holds (the widening to float32 of GMA_float_load_tiff, GMA.c:288-310, then runs on
 * the device): 1 or 2 bytes per pixel cross PCIe instead of 4, and 8-bit DN lands directly in the exact-integer
 * kernel's planes.  Results are identical to widening on the host and calling mimc3_ctx_set_images.
 * Any host pointer works; memory from mimc3_host_alloc (pinned) is DMA'd without the staging copy. */
int mimc3_ctx_set_images_u8(mimc3_ctx *ctx, const uint8_t *i0, const uint8_t *i1, int32_t H, int32_t W);
int mimc3_ctx_set_images_u16(mimc3_ctx *ctx, const uint16_t *i0, const uint16_t *i1, int32_t H, int32_t W);
void *mimc3_host_alloc(size_t bytes);     /* pinned host memory (NULL on failure); read TIFF scanlines straight into it */
void  mimc3_host_free(void *p);
/* Adopt device-resident images (no copy; caller keeps ownership, must outlive the context use). */
int mimc3_ctx_set_images_dev(mimc3_ctx *ctx, const float *d_i0, const float *d_i1, int32_t H, int32_t W);

/* Kernel selection.  By default (mode 0) the library picks, per matcher call:
 *   1 = exact-integer u8 kernel when BOTH resident images were proven (on the device, at set_images
 *       time) to hold only integers in [0,255] -- the 8-bit TIFF case of GMA_float_load_tiff
 *       (GMA.c:288-298) -- and ocw is one of 7, 15, 16, 30, 32, 40;
 *   3 = exact scaled-integer u16 kernel when both images hold only values q/2^s with q < 4096 (12-bit DN,
 *       or what GMA_float_conv2 makes of 8-bit images: integers <= 511 / multiples of 1/8), same ocw set;
 *   4 = the u8 kernel read through per-point offsets, for INTEGER images of kind 3 whose values stay within an
 *       8-bit range locally (the gradient filters of 8-bit images); the few points whose chip or window does
 *       not fit are redone by kernel 3 right behind.  Exact like 3 (same integer sums, rebuilt from q - k);
 *   2 = register-tiled f32 kernel (any f32 imagery, e.g. 16-bit DN) when ocw is one of 7, 15, 16, 30, 32, 40;
 *   5 = the matrix-core form of kernel 1 (dense correlation surfaces on v_mfma_i32_16x16x64_i8), taken first for the
 *       chip sizes it is built for; the points it does not take (null pixels in the window or chip, corridors wider than
 *       its 32 x 32 cell tile, ...) are flagged and done by kernel 1 right behind;
 *   0 = general f32 kernel (any ocw, any window size) otherwise;
 *   6 = the exhaustive search (mimc3_match_ncc_full, mimc3_match_ncc_full_multi, mimc3_match_ncc_pyramid): the matrix-core kernel's surfaces, every point
 *       on the matrix cores (it does not depend on the mode);
 *   7 = the exhaustive search of mimc3_match_ncc_full_planes on a scaled-integer pair: the u16 planes' register-tiled search kernel;
 *   8 = the exhaustive search of mimc3_match_ncc_full_dn on an integral-f32 pair (16-bit DN and its filtered forms): the f32 planes'
 *       search kernel;
 *   9 = the exhaustive search of mimc3_match_ncc_full_any on any other f32 pair (non-integral pixels, NaN or negative nulls), or on any
 *       pair with its mode 1: the float search kernel on the f32 planes, without tables;
 *  10 = the exhaustive search beyond +-15 px (mimc3_match_ncc_wide at R >= 16): the wide float search kernel on the same planes.
 *  11 = the exhaustive search at any chip half-width 1..80 (mimc3_match_ncc_full_chip with its mode 1, or with an ocw that is not one of
 *       the six): the run-time-ocw float search kernel on the same planes, the chip walked in bands of chip rows.
 *  12 = the exhaustive search of mimc3_match_ncc_full_chip_class on an 8-bit pair, with its mode 1 or with an ocw that is not one of the
 *       six: the run-time-ocw matrix-core search kernel on the u8 planes and their tables.
 *  13 = the exhaustive search of mimc3_match_ncc_full_chip_planes on a scaled-integer pair (12-bit DN, a filtered 8-bit pair) with an ocw that
 *       is not one of the six, or on an 8-bit or scaled-integer pair with its mode 1: the run-time-ocw matrix-core search kernel on the u16
 *       planes (two 6-bit planes per pixel) and their tables.
 *  14 = the exhaustive search beyond +-15 px of mimc3_match_ncc_wide_class on an 8-bit pair (R >= 16): the matrix-core wide search kernel on
 *       the u8 planes and their tables, at any chip half-width 1..80.
 *  15 = the exhaustive search beyond +-15 px of mimc3_match_ncc_wide_planes on a scaled-integer pair (R >= 16), or on an 8-bit or
 *       scaled-integer pair with its mode 1: the matrix-core wide search kernel on the u16 planes (two 6-bit planes per pixel) and their
 *       tables, at any chip half-width 1..80.
 *  16 = the exhaustive search beyond +-15 px of mimc3_match_ncc_wide_chip (R >= 16) with its mode 1, or in mode 0 on a pair and at an
 *       (ocw, R) no other wide kernel takes: the run-time-ocw wide float search kernel on the f32 planes, at any chip half-width 1..80.
 * All three give results bit-identical to the reference on integral-DN data.  mode 1 forces kernel 0,
 * mode 2 skips the integer kernels, mode 3 skips only the u8 kernel, mode 4 is mode 0 without kernel 5 (tests use
 * them to cover every kernel on 8-bit inputs too).
 * mimc3_ctx_last_path returns the kernel of the last call (<0 = none yet). */
int mimc3_ctx_set_path(mimc3_ctx *ctx, int32_t mode);
int mimc3_ctx_last_path(mimc3_ctx *ctx);

/* ---- a2: DLC pivot generator.  Replaces get_uv_pivot (MIMC_module.h:41, MIMC_module.c:543-602).
 *      Host code (libm-exact float/double mix of the reference).  Two-call protocol: pass
 *      piv_uv=NULL to get the total pivot count in *total and piv_off filled; then call again
 *      with capacity `cap` (pairs).  MIMC3_EBOUNDS if any point gets zero pivots. ------------- */
int mimc3_get_uv_pivot(const double *xyuvav, int32_t N, float dt, float mpp, float aw_sf, float aw_cre,
                       int32_t ocw, int32_t H, int32_t W,
                       int64_t *piv_off /*[N+1]*/, int32_t *piv_uv /*[cap][2] or NULL*/, int64_t cap,
                       int64_t *total);

/* ---- a3-a7: matcher.  Replaces matching_ncc_dlc_2 (MIMC_module.h:46, MIMC_module.c:805-842)
 *      including extract_refchip/extract_sarea/investigate_valid_grid/find_ncc_peak.
 *      out [N][3] = (du, dv, ncc_peak); invalid point = (NaN, NaN, -3)   (MIMC_module.c:685-687).
 *      `swap` != 0 matches i1 -> i0 (the CLI's "swapped forward" pass, MIMC_main.c:284): the
 *      caller still negates offset, pivots and the resulting (du,dv) exactly as main() does. --- */
int mimc3_match_ncc_dlc(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                        const int32_t *piv_uv, const int64_t *piv_off, int32_t ocw, int32_t swap,
                        float *out /*[N][3] host*/);

/* Device-resident variant used by bench.py and the multi-GPU shard path: all pointers are device
 * pointers; `max_abs_piv_u/v` = max over points of |last pivot| per axis (sizes the LDS window;
 * mimc3_pivot_extent() computes it from a host CSR).  Enqueues on `stream`, no sync. */
int mimc3_match_ncc_dlc_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                            const int32_t *d_piv_uv, const int64_t *d_piv_off, int32_t max_npiv,
                            int32_t max_abs_piv_u, int32_t max_abs_piv_v, int32_t ocw, int32_t swap,
                            float *d_out, void *stream);
int mimc3_pivot_extent(const int32_t *piv_uv, const int64_t *piv_off, int32_t N,
                       int32_t *max_npiv, int32_t *max_abs_u, int32_t *max_abs_v);

/* ---- Exhaustive-search NCC offsets with peak quality (no reference counterpart: the complement of the DLC matcher that
 *      find_ncc_peak's TODOs ask for, MIMC_module.c:649,790, and the AMPCOR-style record MIMC_single_match.c:1-27 promises).
 *
 *   Inputs, for grid point i:
 *     uv0 = ((int)xyuvav[i][2], (int)xyuvav[i][3]);
 *     chip: (2 ocw + 1)^2 pixels of i0 centred at uv0, as extract_refchip cuts it (:845-855);
 *     search centre c = uv0 + offset + shift[i], shift an optional int32 [N][2] (NULL = zero);
 *     integer offsets s = (su, sv) in [-R, R]^2, 1 <= R <= 15;
 *     swap = 1 exchanges the roles of i0 and i1, as in the DLC entry.
 *   Per-cell NCC(s): the reference's cell formula (:719-734) -- null exclusion at MIN_DN, f64, no contraction, cast to f32 --
 *     of the chip with the box of i1 centred at c + s.  Box pixels outside the image are 0, i.e. nulls.  Unlike the DLC window
 *     there is no never-written last row or column: the box is the plane itself.
 *   Per-point outcome:
 *     validity  investigate_valid_grid's rule (:605-644, f32 ratios, > 0.8) on the chip and on the whole (2R + 2 ocw + 1)^2
 *               search box; if either fails the status is -3;
 *     peak      the largest finite NCC(s); on ties the lowest k = (su + R)(2R + 1) + (sv + R) wins (u outer, v inner, as the
 *               reference's 3x3 scan); NaN never wins; no finite cell: status -2;
 *     border    |su| = R or |sv| = R at the peak: status -4 (no fit);
 *     fit       otherwise the reference's 3x3 quadratic fit (:757-788) with its float/double mix, exactly:
 *               c0..c5 = (f32 expressions of the 9 cells) / 36 in f64 (c5 = (-4 n0 + 8 n1 - 4 n2 + 8 n3 + 20 n4 + 8 n5 - 4 n6
 *               + 8 n7 - 4 n8) / 36, the constant of the same fit), du' = (float)((double)(float)(-2 c2 c3 + c1 c4) / det),
 *               det = 4 c0 c2 - c1^2, dv' likewise with (-2 c0 c4 + c1 c3).
 *   Output, f32 [N][8] per point:
 *     0, 1  du, dv = du' + (float)(su + shift_u), dv' + (float)(sv + shift_v): the displacement relative to uv0 + offset, like
 *           columns 0 and 1 of the DLC matcher.  NaN when the status is negative.
 *     2     ncc_peak: the peak cell's f32 NCC, or the status -2 / -3 / -4
 *     3     ncc_fit: the fitted quadratic's value at its extremum (f64: x* = (-2 c2 c3 + c1 c4) / det, y* = (-2 c0 c4 + c1 c3) / det,
 *           c0 x*^2 + c1 x* y* + c2 y*^2 + c3 x* + c4 y* + c5), stored as f32
 *     4     snr: ncc_peak^2 / mean(NCC^2) over the finite cells outside the 3x3 block around the peak (f64, stored as f32; NaN if
 *           there are none)
 *     5-7   the fit's Hessian 2 c0, c1, 2 c2 (h_uu, h_uv, h_vv): the peak-sharpness input of a covariance
 *     Columns 3-7 are NaN when the status is negative.
 *   Refusals: ocw outside {7, 15, 16, 30, 32, 40} or R outside 1..15: MIMC3_EINVAL; a chip that leaves the image, or a search box
 *   beyond the planes' 256-px zero border: MIMC3_EBOUNDS; a pair that did not classify as 8-bit (u8 planes): MIMC3_EUNSUPPORTED.
 *   mimc3_ctx_last_path reports 6.  (mimc3_match_ncc_full_planes is this search on scaled-integer pairs too.) */
int mimc3_match_ncc_full(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                         const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t swap, float *out /*[N][8] host*/);
/* Device-resident variant: d_xyuvav [N][6], d_shift [N][2] or NULL, d_out [N][8] device pointers; enqueues on `stream`, no sync.
 * The caller guarantees the bounds the host entry checks (a point that breaks them gets an all-NaN record and no read). */
int mimc3_match_ncc_full_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                             const int32_t *d_shift, int32_t ocw, int32_t R, int32_t swap, float *d_out, void *stream);

/* ---- Exhaustive search with candidates: the K best correlation peaks of every point, in the layout the post-matcher chain reads
 *      (mimc3_cluster_candidates -> dpf0 -> dpf1 -> QM, mimc3_postprocess: dp [ndp][N][3] with ndp = npeaks, or several calls'
 *      candidates stacked, ndp <= 64).
 *
 *   Inputs, surface, validity and the [N][8] record `out`: exactly mimc3_match_ncc_full's -- the same code computes the record, bit
 *     for bit, the SNR included.  1 <= npeaks <= 8.
 *   Local maximum: a cell s = (su, sv) with
 *     |su| < R and |sv| < R (a border cell is never a candidate, but it takes part as a neighbour);
 *     NCC(s) finite;
 *     for each of its 8 neighbours t: NCC(t) is not finite, or NCC(s) > NCC(t), or NCC(s) == NCC(t) and k(s) < k(t), with
 *     k = (su + R)(2R + 1) + (sv + R) as in the arg-max rule (a flat top yields one local maximum: its lowest k).
 *   Rank: the local maxima by NCC descending, ties by ascending k; candidate j is the j-th of them.
 *   Output cand, f32 [npeaks][N][3], pass-major: cand[j][i] = (du, dv, ncc) of point i's candidate j:
 *     ncc     the cell's f32 NCC;
 *     du, dv  the reference's 3x3 fit around that cell, the float/double expression sequence of the record's fit, plus
 *             (float)(su + shift_u), (float)(sv + shift_v); a non-finite neighbour makes the fit NaN, as in the record.
 *   Slots without a peak:
 *     fewer than npeaks local maxima: the remaining slots are (NaN, NaN, -2);
 *     status -3 (validity): every slot is (NaN, NaN, -3), the DLC matcher's invalid match;
 *     a point that gets the all-NaN record (the _dev entry's contract): every slot all NaN.
 *     None of these passes clustering's ncc > 0.1 test.
 *   Consequences:
 *     where the record has a fit (its peak is interior), candidate 0 equals the record's columns 0-2 bit for bit;
 *     where the record has status -4 (peak on the border), the candidates are the interior local maxima that exist;
 *     status -2 (no finite cell): no local maximum, every slot (NaN, NaN, -2);
 *     at R = 1 there is one interior cell, so at most one candidate.
 *   Refusals: npeaks outside 1..8: MIMC3_EINVAL; every refusal of mimc3_match_ncc_full, unchanged.  mimc3_ctx_last_path reports 6.
 *   (mimc3_match_ncc_full_planes returns the same candidates on scaled-integer pairs too.) */
int mimc3_match_ncc_full_multi(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                               const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap,
                               float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host*/);
/* Device-resident variant: as mimc3_match_ncc_full_dev, plus d_cand [npeaks][N][3]; enqueues on `stream`, no sync. */
int mimc3_match_ncc_full_multi_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                   const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                   float *d_cand, void *stream);

/* ---- Exhaustive search on the planes the context matches on: 8-bit pairs and scaled-integer pairs (12-bit DN; an 8-bit pair after
 *      mimc3_ctx_filter_images: gradients, Laplacian) -- the variants the post-matcher chain chooses among.
 *
 *   A superset of the two entries above.  npeaks = 0: the record alone (cand NULL), word for word mimc3_match_ncc_full; npeaks in
 *   1..8: the record and cand [npeaks][N][3], word for word mimc3_match_ncc_full_multi -- validity, first-wins arg-max, border rule,
 *   fit, SNR, Hessian, local-maximum rule and rank, the encodings of empty slots.  It runs on the pair the context currently matches on:
 *     8-bit pair       the matrix-core kernels of the entries above; results bit for bit theirs.  mimc3_ctx_last_path reports 6.
 *     scaled-integer   (every pixel q / 2^s with q < 4096, s = 0 or 3 per image: the pairs the DLC matcher runs on u16 planes) the
 *                      search runs on the u16 planes q.  A pixel is null exactly when q == 0; box pixels outside the image are the
 *                      256-px zero border.  mimc3_ctx_last_path reports 7.
 *                      The integers need no new arithmetic: every f32 product of two pixels q_a / 2^sa * q_b / 2^sb is exact (< 2^24
 *                      significant bits), every f64 sum is an exact integer times a power of two, n sxy - sx sy and both variance
 *                      terms are exact (< 2^50), and the scale 2^-(sa + sb) commutes with the rounding of the variance product, with
 *                      the square root (an even exponent) and with the division -- the reference's cell formula on the float pixels
 *                      equals the same formula on the integers q bit for bit.  The record and the candidates come from the same
 *                      code as on 8-bit pairs.
 *     anything else    (16-bit DN, non-integral data, NaN nulls) MIMC3_EUNSUPPORTED.  (mimc3_match_ncc_full_dn takes 16-bit DN.)
 *   Refusals: npeaks outside 0..8, or cand NULL with npeaks > 0 / not NULL with npeaks = 0: MIMC3_EINVAL; ocw, R, a chip that leaves
 *   the image, a search box beyond the zero border: as mimc3_match_ncc_full.  (mimc3_match_ncc_pyramid_dn is the coarse-to-fine search on these pairs.) */
int mimc3_match_ncc_full_planes(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                                const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                                int32_t swap, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/);
/* Device-resident variant: enqueue only, the contract of mimc3_match_ncc_full_multi_dev (d_cand NULL iff npeaks == 0). */
int mimc3_match_ncc_full_planes_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                    const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                    float *d_cand, void *stream);

/* ---- Exhaustive search on every pair the planes' matchers take: the two classes above and integral-f32 pairs -- 16-bit DN (Landsat 8/9
 *      OLI, Sentinel-2) and what mimc3_ctx_filter_images makes of it.
 *
 *   A superset of mimc3_match_ncc_full_planes: its arguments, checks, record, candidates, statuses and empty-slot encodings word for
 *   word, with one more class.  It runs on the pair the context currently matches on:
 *     8-bit pair       as mimc3_match_ncc_full_planes; results bit for bit.  mimc3_ctx_last_path reports 6.
 *     scaled-integer   as mimc3_match_ncc_full_planes; results bit for bit.  mimc3_ctx_last_path reports 7.
 *     integral f32     (every pixel w / 2^s with w an integer in [0, 2^20), s = 0 or 3 per image, and the pair in neither class above)
 *                      the search runs on the zero-bordered f32 planes and their 16-byte summed-area tables (sum w | nulls << 40,
 *                      sum fl(w w)), built on the first call that needs them and kept until the pair changes.  A pixel is null
 *                      exactly when it is 0 (MIN_DN = 1e-10 lies below 1/8); box pixels outside the image are the 256-px zero border.
 *                      mimc3_ctx_last_path reports 8.
 *                      The cell is the one defined above, the reference's (MIMC_module.c:719-734): f32 pixel products, f64 sums, the
 *                      f64 expression without contraction, cast to f32.  On this class the f32 product ROUNDS (w_a w_b reaches 2^40,
 *                      an f32 holds 24 bits), and that rounding is part of the result: sxx, syy and sxy are sums of
 *                      (double)(float)(a * b), not of exact products.  What stays exact: fl(w_a w_b) is an integer below 2^40 and
 *                      a chip has at most 6,561 pixels, so every f64 sum is an exact integer below 2^53 in any order; and the
 *                      scales 2^-s commute with the product's rounding and with every later operation (the square root sees the
 *                      even exponent 2 (sa + sb), the division cancels it), so the kernel works on the integers w alone.  What does
 *                      not: n sxy, sx sy and the variance terms pass 2^53 (up to about 2^57) and round, so the finish performs
 *                      the reference's operations one by one -- each product, each difference, the variance product, sqrt, the
 *                      division, all correctly rounded f64 -- and not the reciprocal-square-root shortcut of the other classes,
 *                      whose guard was argued for exact inputs.  The record and the candidates come from the same code as on
 *                      every other class.
 *     anything else    (non-integral data, NaN nulls, values of 2^20 and above) MIMC3_EUNSUPPORTED.  (mimc3_match_ncc_full_any takes it.)
 *   Refusals: those of mimc3_match_ncc_full_planes; a chip-atlas context: MIMC3_ESTATE.  (mimc3_match_ncc_pyramid_dn is the coarse-to-fine search on these pairs.) */
int mimc3_match_ncc_full_dn(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                            const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                            int32_t swap, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_planes_dev.  (The first call on an integral-f32 pair builds its planes
 * and tables on the context's own stream and waits for them before it enqueues on `stream`.) */
int mimc3_match_ncc_full_dn_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                float *d_cand, void *stream);

/* ---- Exhaustive search on ANY f32 pair: non-integral pixels (SAR amplitude or sigma-0, high-pass or Wallis filtered optical pairs,
 *      reflectance), NaN or negative nulls (GeoTIFF no-data NaN or -9999).  The arguments of mimc3_match_ncc_full_dn plus `mode` and `surf`.
 *
 *   mode 0   dispatch by the class of the pair the context currently matches on: 8-bit, scaled-integer and integral-f32 pairs go where
 *            mimc3_match_ncc_full_dn sends them (mimc3_ctx_last_path 6, 7, 8), bit for bit; every other f32 pair runs the float kernel
 *            (match_full_f32g_kernel.hip) on the zero-bordered f32 planes, without tables.  mimc3_ctx_last_path reports 9.
 *   mode 1   the float kernel on any pair, whatever its class (tests; and this entry's only way to the surfaces of an integer-class
 *            pair -- mimc3_match_ncc_full_surf below returns them from the class kernels).
 *   Any other mode: MIMC3_EINVAL.
 *   surf     optional (NULL: none), f32 [N][(2R+1)^2]: every point's NCC surface in k order, k = (su + R)(2R + 1) + (sv + R); all NaN at
 *            status -3 (and for a point of the _dev entry that breaks the bounds).  Only the float kernel serves it: surf != NULL on a
 *            call the float kernel does not run is MIMC3_EINVAL.
 *   out, cand   exactly the record and the candidates of mimc3_match_ncc_full_dn: statuses -2 / -3 / -4, the local-maximum rule, the
 *            rank, the fit.  Refusals as there (ocw one of 7, 15, 16, 30, 32, 40; 1 <= R <= 15; npeaks 0..8 and cand NULL iff npeaks == 0;
 *            MIMC3_EBOUNDS; a chip-atlas context: MIMC3_ESTATE).  The older entries keep refusing this class (MIMC3_EUNSUPPORTED).
 *
 *   The cell on float pixels is the reference's, literally (MIMC_module.c:605-644, :719-734), with its TWO null rules, which differ on NaN:
 *     validity   counts the pixels with p < MIN_DN (MIN_DN = 1e-10, compared in double) in the chip and in the whole (2R + 2 ocw + 1)^2
 *                box, pixels outside the image being 0; the point gets status -3 when either f32 ratio exceeds 0.8.  A NaN pixel is
 *                NOT counted (NaN < x is false): a chip of NaN alone is valid, and has no cell (-2).
 *     inclusion  a pixel pair enters a cell's sums when a >= MIN_DN && b >= MIN_DN.  A NaN pixel IS excluded (NaN >= x is false), as
 *                are 0, -0.0, negatives and positives below 1e-10.  An included +Inf, or a product that overflows, goes through the
 *                arithmetic as in the reference (the cells that contain it are not finite; no other cell sees it).
 *     terms      n counts the included pairs; sx, sy add (double)a, (double)b; sxx, syy, sxy add (double)(float)(a a), (double)(float)(b b),
 *                (double)(float)(a b): f32 products, widened.
 *     finish     the reference's f64 operations one by one, correctly rounded (no reciprocal-square-root shortcut), cast to f32.
 *   Order, and its bound.  On the integer classes every partial sum is an exact integer and any order gives the reference's bits.  Float
 *   terms do not have that, so: each of the five sums is the f64 sum of exactly those terms in an order the kernel chooses; the order is
 *   a function of (ocw, R, npeaks == 0) alone, so a call is deterministic run to run; and the sums are formed by ADDITIONS ONLY -- no
 *   running sum that subtracts, no summed-area difference.  Every included term is positive (pixels >= 1e-10), so an additions-only f64
 *   sum of m <= 6,561 terms has a relative error of at most (m - 1) 2^-53 < 7.3e-13 in ANY order: the kernel's sums and the
 *   reference's (pixel order) differ by at most twice that, some 2^-39 -- against the 2^-24 of an f32 ulp.  Where the cell's expression
 *   is well conditioned (a textured chip: the variances are not differences of nearly equal numbers) the f32 cell differs from the
 *   reference's by at most 1 ulp, and on well under 1 % of the cells.  Everything after the surface -- arg-max, border test, fit, SNR,
 *   Hessian, local maxima, rank -- is a deterministic function of the surface's f32 values.
 *   On an integer-class pair every sum is exact in any order and the finish is the reference's: mode 1 returns the bytes of
 *   mimc3_match_ncc_full_dn.
 *   (mimc3_match_ncc_pyramid_any is the coarse-to-fine search on these pairs.)
 *   Out of scope here: several GPUs, MIMC3_hip_offsets on float TIFFs, and any tuning of the float kernel beyond its first form. */
int mimc3_match_ncc_full_any(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                             const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                             int32_t swap, int32_t mode, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                             float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_dn_dev; d_surf device memory or NULL.  (The first call on a pair builds
 * its f32 planes on the context's own stream and waits for them before it enqueues on `stream`.) */
int mimc3_match_ncc_full_any_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                 const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *d_out,
                                 float *d_cand, float *d_surf, void *stream);

/* ---- The surfaces from the kernel of the pair's class: the dispatch of mimc3_match_ncc_full_any(mode 0) with surf MANDATORY and served by
 *      whichever kernel runs -- the matrix-core kernel on an 8-bit pair, the u16 and integral-f32 kernels on theirs (each in a form that
 *      also stores the finished surface it holds in LDS), the float kernel on every other pair.  What a stack layer needs
 *      (mimc3_stack_add_class), at the cost of the class's own search plus the surface writes.
 *
 *   Arguments   those of mimc3_match_ncc_full_any without `mode`.  1 <= R <= 15, npeaks 0..8, cand NULL iff npeaks == 0.
 *   out, cand   exactly the record and the candidates of mimc3_match_ncc_full_dn on an integer-class pair (of mimc3_match_ncc_full_any
 *               on a float pair), bit for bit.  mimc3_ctx_last_path reports 6 / 7 / 8 / 9 as the dispatch decides.
 *   surf        f32 [N][(2R+1)^2] in k order, k = (su + R)(2R + 1) + (sv + R); all NaN at status -3 (and for a point of the _dev entry
 *               that breaks the bounds).  On an integer-class pair every sum is an exact integer in any order and every kernel finishes a
 *               cell with the reference's operations, so the surface equals that of mimc3_match_ncc_full_any(mode 1, surf) cell for cell
 *               AS F32 VALUES: finite cells are bit for bit, a non-finite cell is of the same kind (NaN, +Inf or -Inf); NaN payload bits
 *               are not part of the contract.  On a float pair the call IS mimc3_match_ncc_full_any(mode 0, surf): the same bytes.
 *   Refusals    surf NULL: MIMC3_EINVAL (with the other arguments); every other refusal is mimc3_match_ncc_full_any's, in its order.
 *   mimc3_match_ncc_full_any itself is unchanged: surf on a call an integer kernel runs stays MIMC3_EINVAL there.
 *   Out of scope: the pyramid entries, several GPUs, MIMC3_hip_offsets. */
int mimc3_match_ncc_full_surf(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                              const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                              int32_t swap, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                              float *surf /*[N][(2R+1)^2] host*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_any_dev without `mode`; d_surf is required. */
int mimc3_match_ncc_full_surf_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                  const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                  float *d_cand, float *d_surf, void *stream);

/* ---- Exhaustive search at ANY chip half-width: 1 <= ocw <= mimc3_full_chip_max_ocw() = 80 -- the reference's other chip sets (7, 10, 15, 11
 *      and 14, 30, 60, 80; MIMC3_DLC.c:140-149) and everything between.  The arguments of mimc3_match_ncc_full_any, `mode` and `surf`
 *      included; 1 <= R <= 15, npeaks 0..8, cand NULL iff npeaks == 0.
 *
 *   mode 0, ocw one of 7, 15, 16, 30, 32, 40   the call IS mimc3_match_ncc_full_any(mode 0): the same bytes, the same mimc3_ctx_last_path
 *            (6 / 7 / 8 / 9), and the same refusal of surf where an integer kernel runs.
 *   mode 0, any other ocw                      the run-time-ocw kernel (match_full_chip_kernel.hip), whatever the pair's class.
 *   mode 1   that kernel at any ocw in range, the six included (tests and timing).  mimc3_ctx_last_path reports 11 when it ran.
 *   Any other mode: MIMC3_EINVAL.
 *   When that kernel runs the definition is that of mimc3_match_ncc_full_any in mode 1, word for word (see there): the zero-bordered f32
 *   planes whatever the pair's class; both null rules (validity over the chip and over the whole (2R + 2 ocw + 1)^2 box, status -3 above a
 *   ratio of 0.8, a NaN not counted; inclusion a >= 1e-10 && b >= 1e-10, a NaN excluded); the terms (f32 products widened to f64) and
 *   sums formed by additions only; the reference's f64 finish, correctly rounded; the first-wins arg-max in k = (su + R)(2R + 1) +
 *   (sv + R); statuses -2 / -3 / -4, the 3 x 3 fit, ncc_fit, SNR and the Hessian; the local-maximum rule and its rank; surf [N][(2R+1)^2]
 *   in k order, all NaN at status -3 and for a point of the _dev entry that breaks the bounds (chip outside the image, box outside the
 *   256-px zero border): that point's record is all NaN and each of its candidate slots is (NaN, NaN, NaN), as in
 *   mimc3_match_ncc_full_any_dev.
 *   Term bound.  A sum has m <= 25,921 (161^2) positive terms, so an additions-only f64 sum is within (m - 1) 2^-53 < 2.9e-12
 *   (relative) of the exact sum in ANY order -- against the 6e-8 of an f32 ulp.
 *   Order of the additions.  The chip is walked in bands of mimc3_full_chip_band_rows(ocw, R) chip rows (the whole chip where it fits 79 KB
 *   of LDS with its box; ocw <= 41 at R 15).  A band without an excluded pixel in its chip rows and the box rows they meet runs the clean
 *   body, any other the masked body; the order is fixed for given (ocw, R, npeaks == 0) and for which body runs in which band.  It never
 *   depends on N, on the point's place in the grid, or on timing.  No float atomics.
 *   Exactness.  Every partial sum is an exact integer (times a power of two) while m * (largest f32 product) < 2^53.  That holds for
 *   8-bit, 12-bit and 16-bit DN (and their x 1/8 filtered forms) at every ocw up to 80: 2^32 * 25,921 < 2^47.  There the surface is the
 *   reference-order sums' bit for bit, and at one of the six ocw the bytes of mimc3_match_ncc_full_any(mode 1).  For integral-f32 pixels
 *   near 2^20 at the largest chips (2^40 * 25,921 > 2^53) it no longer holds and the float bound above applies: the bytes of
 *   mimc3_match_ncc_full_dn are NOT promised there.
 *   Refusals    those of mimc3_match_ncc_full_any, in its order, with "ocw must be in 1..80" in place of the six-ocw text.  Every older
 *   entry keeps its six-ocw refusal.
 *   mimc3_full_chip_band_rows(ocw, R)   the band height the launch uses (chip rows; 2 ocw + 1 = one band); 0 outside ocw 1..80, R 1..15.
 *   Out of scope: the u16 and integral-f32 class kernels at other chip sizes -- a 16-bit pair at ocw 10 pays the float kernel (an
 *   8-bit pair has mimc3_match_ncc_full_chip_class below); mimc3_match_ncc_wide, the pyramids, forward-backward and mimc3_stack_add / _add_class / _add_scaled at other chip sizes
 *   (mimc3_stack_add_surfaces takes this entry's surfaces as they are); several GPUs; MIMC3_hip_offsets on float TIFFs; ocw above 80. */
int mimc3_full_chip_max_ocw(void);
int mimc3_full_chip_band_rows(int32_t ocw, int32_t R);
int mimc3_match_ncc_full_chip(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                              const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                              int32_t swap, int32_t mode, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                              float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_any_dev. */
int mimc3_match_ncc_full_chip_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                  const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *d_out,
                                  float *d_cand, float *d_surf, void *stream);

/* ---- Exhaustive search at any chip half-width with the 8-BIT pair on the matrix cores: the arguments of mimc3_match_ncc_full_chip, `mode`,
 *      `cand` and `surf` (both optional) included; 1 <= ocw <= 80, 1 <= R <= 15, npeaks 0..8, cand NULL iff npeaks == 0.
 *
 *   mode 0, ocw one of 7, 15, 16, 30, 32, 40   the class dispatch of mimc3_match_ncc_full_any(mode 0): the same record and candidates, the same
 *            mimc3_ctx_last_path (6 / 7 / 8 / 9); surf, when given, is served as mimc3_match_ncc_full_surf serves it (by whichever kernel runs).
 *   mode 0, any other ocw                      an 8-bit pair runs the run-time-ocw matrix-core kernel (match_full_chip_u8_kernel.hip;
 *            mimc3_ctx_last_path 12); every other class runs the float kernel of mimc3_match_ncc_full_chip (11), with that entry's bytes.
 *   mode 1   the matrix-core kernel at every ocw in range, the six included (tests and timing).  8-bit pairs only: any other pair is
 *            MIMC3_EUNSUPPORTED, where the family refuses a class.
 *   Any other mode: MIMC3_EINVAL.
 *   The kernel.  The exhaustive-search half of the matrix-core matcher with ocw as a kernel argument: the Toeplitz-band GEMM on
 *   v_mfma_i32_16x16x64_i8 over the 32 x 32 cell tile with origin c - R, the window-side box sums on the same pipe, the chip's sums from
 *   the packed table in sub-boxes of at most 64 x 64 pixels (one query is exact only up to 8,224 pixels: ocw >= 45 would carry between
 *   its fields on near-saturated data), the guarded fast finish with its exact redo and the tails of the family.  Two forms: the clean one
 *   runs over all points and flags those that hold a null (pixel 0) in the chip or the search box; the masked one runs behind it over the
 *   flagged points and takes any null pattern -- the five masked sums are the clean ones minus correlations with the two null indicators,
 *   whose operands it forms in registers, so it needs no further LDS and is not banded.  Every sum is an exact i32 (the largest true sum
 *   is 161^2 255^2 < 2^31).
 *   Promise on an 8-bit pair.  Every sum of mimc3_match_ncc_full_chip's float kernel is the same exact integer there, so record, candidates
 *   and surface are the bytes of mimc3_match_ncc_full_chip(mode 1) at every ocw 1..80, and at the six also those of
 *   mimc3_match_ncc_full_surf: finite surface cells bit for bit, a non-finite cell of the same kind (NaN, +Inf or -Inf; payload bits are
 *   not part of the contract); statuses, the all-NaN surface at -3 and the all-NaN results of a _dev point that breaks the bounds included.
 *   Dispatch.  mode 0 sends an ocw to the matrix-core kernel where every pass of its timing series was faster than every pass of the float
 *   kernel's (tools/full_chip_u8_time.py, BASELINE C2; profiles/full_search_chip_u8/): every ocw measured, 7 .. 80, those where 97-99.6 %
 *   of the points run the masked form included.  No range is kept on the float kernel.
 *   mimc3_full_chip_class_layout(ocw, out)   the kernel's layout at this ocw: out[0] K chunks of 64 window columns per chip row (1..3),
 *            out[1] 16-row tiles and out[2] K chunks of the box sums, out[3] dynamic LDS bytes; returns 1, or 0 outside ocw 1..80.
 *   Refusals    those of mimc3_match_ncc_full_chip, in its order; mode 1 on a pair that is not 8-bit: MIMC3_EUNSUPPORTED.
 *   mimc3_match_ncc_full_chip and every older entry are unchanged.
 *   Out of scope: u16 (mimc3_match_ncc_full_chip_planes below) and integral-f32 kernels at other chip sizes; the wide search, the pyramids, forward-backward and mimc3_stack_add* at
 *   other chip sizes (mimc3_stack_add_surfaces takes this entry's surfaces as they are); several GPUs. */
int mimc3_full_chip_class_layout(int32_t ocw, int32_t out[4]);
int mimc3_match_ncc_full_chip_class(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                                    const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                                    int32_t swap, int32_t mode, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                                    float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_chip_dev. */
int mimc3_match_ncc_full_chip_class_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                        const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *d_out,
                                        float *d_cand, float *d_surf, void *stream);

/* ---- Exhaustive search at any chip half-width with the 8-BIT AND THE SCALED-INTEGER pair on the matrix cores: the arguments of
 *      mimc3_match_ncc_full_chip_class.  A scaled-integer pair is what mimc3_match_ncc_full_planes takes: pixels q / 2^s with q < 4096 on u16
 *      planes -- 12-bit DN, and the d/dx, d/dy and Laplacian forms of an 8-bit pair (mimc3_ctx_filter_images).
 *
 *   mode 0, ocw one of 7, 15, 16, 30, 32, 40   the class dispatch, exactly as mimc3_match_ncc_full_chip_class(mode 0).
 *   mode 0, any other ocw                      an 8-bit pair runs the u8 matrix-core kernel (mimc3_ctx_last_path 12); a scaled-integer pair runs
 *            the run-time-ocw matrix-core kernel on the u16 planes (match_full_chip_u16_kernel.hip; 13) at the chip sizes the measured rule
 *            below names; every other class runs the float kernel of mimc3_match_ncc_full_chip (11).
 *   mode 1   the u16 matrix-core kernel at every ocw in range, the six included, on any pair that is 8-bit (q < 256 on its u16 planes) or
 *            scaled-integer; any other pair is MIMC3_EUNSUPPORTED, where the family refuses a class.
 *   Any other mode: MIMC3_EINVAL.
 *   The kernel.  mimc3_match_ncc_full_chip_class's, with every pixel as two 6-bit planes q = 64 h + l: both are non-negative i8 values, so the
 *   Toeplitz-band GEMM on v_mfma_i32_16x16x64_i8 needs no offset terms, and sum ab = 4096 HH + 64 (SS - HH - LL) + LL from three
 *   correlations per K chunk (SS that of the plane sums h + l <= 126), put together in 64 bits (the true sum reaches 161^2 4095^2 < 2^39).
 *   The window-side box sums run on the same pipe (row sums of q as three byte planes, of q^2 -- a u32 -- as four), the chip's sums come from
 *   the packed u16 table in sub-boxes of at most 64 x 64 pixels (one query is exact only while sum q < 2^25: ocw >= 45 would carry on
 *   near-saturated data), the null counts from the u32 null table.  Two forms as there: the clean one flags the points that hold a null
 *   (q == 0) in the chip or the search box, the masked one takes any null pattern behind it, its extra operands formed in registers.
 *   The cell is finished with the float kernel's own f64 operations on the exact integer sums: from ocw 76 on n sum ab and (sum a)^2 can
 *   pass 2^53 on near-saturated 12-bit data and round -- identically in both kernels.
 *   Promise on an 8-bit or scaled-integer pair.  Record, candidates and surface are the bytes of mimc3_match_ncc_full_chip(mode 1) at every
 *   ocw 1..80; at the six also those of mimc3_match_ncc_full_planes / mimc3_match_ncc_full_surf (finite surface cells bit for bit, a
 *   non-finite cell of the same kind); on an 8-bit pair those of mimc3_match_ncc_full_chip_class(mode 1).  Statuses, the all-NaN surface at
 *   -3 and the all-NaN results of a _dev point that breaks the bounds included.
 *   Dispatch.  mode 0 sends an ocw to the u16 matrix-core kernel where every pass of its timing series was faster than every pass of the
 *   float kernel's in the same session (tools/full_chip_u16_time.py; profiles/full_search_chip_u16/): every ocw measured, 7 .. 80, on C2 as
 *   12-bit DN and as its d/dx pair, those where 97-99.6 % of the points run the masked form included.  No range is kept on the float kernel.
 *   mimc3_full_chip_planes_layout(ocw, out)   the kernel's layout at this ocw: out[0] K chunks of 64 window columns per chip row (1..3),
 *            out[1] 16-row tiles and out[2] K chunks of the box sums, out[3] dynamic LDS bytes; returns 1, or 0 outside ocw 1..80.
 *   Refusals    those of mimc3_match_ncc_full_chip_class, in its order; mode 1 on a pair that is neither 8-bit nor scaled-integer:
 *   MIMC3_EUNSUPPORTED.  mimc3_match_ncc_full_chip, mimc3_match_ncc_full_chip_class and every older entry are unchanged.
 *   Out of scope: the integral-f32 kernel (16-bit pairs) at other chip sizes; the wide search, the pyramids, forward-backward and
 *   mimc3_stack_add* at other chip sizes (mimc3_stack_add_surfaces takes this entry's surfaces as they are); several GPUs. */
int mimc3_full_chip_planes_layout(int32_t ocw, int32_t out[4]);
int mimc3_match_ncc_full_chip_planes(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                                     const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                                     int32_t swap, int32_t mode, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                                     float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_chip_dev. */
int mimc3_match_ncc_full_chip_planes_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                         const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *d_out,
                                         float *d_cand, float *d_surf, void *stream);

/* ---- Exhaustive search beyond +-15 px: ONE exact pass at full resolution over a search range of up to +-47 px, with candidates from the
 *      whole range -- for a displacement the a-priori shift misses by more than 15 px, which the entries above return as status -4 or
 *      as a confident wrong peak, and which the pyramid reaches only by deciding on reduced images.
 *
 *   The definition is that of mimc3_match_ncc_full_any in mode 1, word for word (see there), with 1 <= R <= mimc3_wide_max_radius(ocw):
 *   every pair runs on its zero-bordered f32 planes whatever its class; the two null rules (validity over the chip and over the whole
 *   (2R + 2 ocw + 1)^2 box, status -3 above a ratio of 0.8; inclusion a >= 1e-10 && b >= 1e-10); the terms (f32 products widened to f64,
 *   additions only) and the finish (the reference's f64 operations, correctly rounded); the first-wins arg-max in k = (su + R)(2R + 1) +
 *   (sv + R); statuses -2 / -3 / -4, the 3 x 3 fit, ncc_fit, the Hessian, SNR; the local-maximum rule and the rank of the candidates; surf
 *   [N][(2R+1)^2] in k order, all NaN at status -3; MIMC3_EBOUNDS (the search box must stay inside the planes' 256-px zero border) and
 *   MIMC3_ESTATE as there.  The order of a float sum is the kernel's own, a function of (ocw, R, npeaks == 0) alone, additions only: the
 *   bound (m - 1) 2^-53 of that text holds unchanged, because m <= 6,561 does not depend on R.
 *   R <= 15    IS mimc3_match_ncc_full_any(mode 1): the same kernel, the same bytes.  mimc3_ctx_last_path reports 9.
 *   R >= 16    the wide kernel (match_wide_kernel.hip).  mimc3_ctx_last_path reports 10.
 *   mimc3_wide_max_radius(ocw)   the largest R taken at this chip size: 47 (a 95 x 95 surface) wherever box, chip and surface fit the
 *              160 KB of LDS of a compute unit -- ocw 7, 15, 16, 30, 32 -- and 39 at ocw 40; 0 for an ocw that is not one of the six.
 *   Refusals: R outside 1 .. mimc3_wide_max_radius(ocw), ocw not one of 7, 15, 16, 30, 32, 40, npeaks outside 0..8, cand NULL unless
 *   npeaks == 0: MIMC3_EINVAL; a chip outside the image or a box outside the border: MIMC3_EBOUNDS; no images, or a chip-atlas context:
 *   MIMC3_ESTATE.
 *   mimc3_wide_lds_bytes(ocw, R)   the dynamic LDS (bytes) of the wide kernel's launch at this chip size and radius, from the layout the
 *              launch uses (tools and documents quote it); 0 outside 1 .. mimc3_wide_max_radius(ocw).
 *   The stack takes this range through mimc3_stack_begin_wide, forward-backward consistency through mimc3_match_ncc_wide_fb, and
 *   MIMC3_hip_offsets accepts R up to mimc3_wide_max_radius(ocw) at levels = 1.
 *   Not covered: the pyramid entries keep R <= 15; several GPUs; Context.full_candidates of the Python layer. */
int mimc3_wide_max_radius(int32_t ocw);
int mimc3_wide_lds_bytes(int32_t ocw, int32_t R);
int mimc3_match_ncc_wide(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                         const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                         int32_t swap, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                         float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_any_dev (a point that breaks the bounds gets the all-NaN record, NaN
 * candidate slots and an all-NaN surface). */
int mimc3_match_ncc_wide_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                             const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                             float *d_cand, float *d_surf, void *stream);

/* ---- The exhaustive search beyond +-15 px with the 8-BIT pair on the matrix cores, at ANY chip half-width 1 <= ocw <= 80
 *      (match_wide_u8_kernel.hip): mimc3_match_ncc_wide pays 40 to 400 times the R-15 price of an 8-bit pair (a float kernel, f64 adds) and
 *      takes the six built chip sizes only.
 *   The arguments are those of mimc3_match_ncc_full_chip_class, with 1 <= R <= mimc3_wide_class_max_radius(ocw) (47 for 1 <= ocw <= 80).
 *   R <= 15, any mode   mimc3_match_ncc_full_chip_class with the same mode: its kernel, its bytes, its last_path.
 *   R >= 16, mode 0     an 8-bit pair runs the matrix-core wide kernel, mimc3_ctx_last_path 14 ("u8_mfma_wide"), at every (ocw, R) named by
 *                       the measured rule below and at every (ocw, R) mimc3_match_ncc_wide does not take; any other (ocw, R), and every
 *                       pair of another class, runs mimc3_match_ncc_wide's kernel where that entry takes (ocw, R): its bytes, last_path
 *                       10.  A pair that is not 8-bit at any other (ocw, R): MIMC3_EUNSUPPORTED, at the step where the family refuses a
 *                       class.
 *   R >= 16, mode 1     the matrix-core wide kernel at every (ocw, R) in range, 8-bit pairs only; any other pair: MIMC3_EUNSUPPORTED.
 *   any other mode      MIMC3_EINVAL.  The order of refusals is that of mimc3_match_ncc_full_chip_class.
 *   The kernel.  mimc3_match_ncc_full_chip_class's, over a grid of ceil(S / 32)^2 tiles of 32 x 32 cells, S = 2R + 1 <= 95: per point the
 *   header, the chip's sums from the packed table in 64 x 64 sub-boxes, the null count of the whole (2R + 2 ocw + 1)^2 box, status -3 above
 *   0.8, the chip plane staged once; per tile the window restaged, the Toeplitz-band GEMM on v_mfma_i32_16x16x64_i8, the box sums against
 *   bands of ones, the masked corrections, sum ab in f64, the guarded finish, into a surface at pitch 96 with LDS bytes of its own; cells
 *   beyond S are computed and dropped.  Then mimc3_match_ncc_wide's tails, unmodified.  A clean form over all points flags those with a null
 *   in the chip or the box; a masked form runs behind it over the flagged points.
 *   Promise on an 8-bit pair: record, candidates and surface are the bytes of the definition mimc3_match_ncc_wide states
 *   (mimc3_match_ncc_full_any in mode 1, word for word) -- at the six chip sizes within mimc3_wide_max_radius those of mimc3_match_ncc_wide
 *   itself (finite surface cells bit for bit, a non-finite cell of the same kind); statuses -2 / -3 / -4 and the all-NaN surface at -3 agree.
 *   mimc3_wide_class_layout(ocw, R, out)   the kernel's layout: out[0] K chunks of 64 window columns per chip row (1..3), out[1] cell tiles
 *              per axis (2..3), out[2] threads per workgroup (128), out[3] dynamic LDS bytes, from the constexpr layout the launch uses;
 *              returns 1, or 0 outside 1 <= ocw <= 80, 16 <= R <= 47.
 *   The mode-0 rule: an (ocw, R) goes to the matrix-core kernel where every pass of its series was faster than every pass of the float
 *   wide kernel's in the same session (tools/wide_u8_time.py, profiles/full_search_wide_u8/).  Measured on C2 (189,054 points, one MI355X): true in all 18
 *   configurations the float kernel takes -- ocw 16 at R 16 / 23 / 31 / 32 / 47: 9.73 / 11.01 / 15.76 / 27.28 / 44.61 ms against 103.1 / 196.8 / 387.2 / 464.7 / 1296.8; ocw 7 at R 16 / 47: 5.09 / 29.75 against 19.87 / 276.6;
 *   ocw 40 at R 16 / 39: 51.25 / 221.2 against 1648.0 / 6065.8 -- and in a second run at ocw 15, 30 and 32 (R 16 and 47: 9.4 to 25.8 times faster), so every (ocw, R) that mimc3_match_ncc_wide
 *   takes goes to the matrix-core kernel; ocw 80 at
 *   R 16 / 47, where it is the only kernel: 552.5 / 1411.2 ms.
 *   MIMC3_hip_offsets calls this entry in mode 0 at levels = 1, fb = 0, 16 <= R <= mimc3_wide_max_radius(ocw): the same files, an 8-bit raw
 *   pair on the matrix cores.
 *   12-bit and filtered pairs beyond R 15 on the matrix cores: mimc3_match_ncc_wide_planes, below.
 *   Out of scope: mimc3_stack_add / _add_class, mimc3_match_ncc_wide_fb and
 *   Context.full_candidates through this kernel; an ocw outside the six on the command line at R > 15; the pyramids; several GPUs. */
int mimc3_wide_class_max_radius(int32_t ocw);
int mimc3_wide_class_layout(int32_t ocw, int32_t R, int32_t out[4]);
int mimc3_match_ncc_wide_class(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                               const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                               int32_t swap, int32_t mode, float *out /*[N][8] host*/,
                               float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_chip_class_dev. */
int mimc3_match_ncc_wide_class_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                   const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                   float *d_out, float *d_cand, float *d_surf, void *stream);

/* ---- The exhaustive search beyond +-15 px with the SCALED-INTEGER pair (u16 planes, q < 4096: 12-bit DN, and the d/dx, d/dy and Laplacian
 *      forms of an 8-bit pair) on the matrix cores as well, at ANY chip half-width 1 <= ocw <= 80 (match_wide_u16_kernel.hip).
 *   The arguments are those of mimc3_match_ncc_wide_class: 1 <= ocw <= 80, 1 <= R <= mimc3_wide_class_max_radius(ocw), else MIMC3_EINVAL.
 *   R <= 15, any mode   mimc3_match_ncc_full_chip_planes with the same mode: its kernel, its bytes, its last_path.
 *   R >= 16, mode 1     the matrix-core wide kernel on the u16 planes, mimc3_ctx_last_path 15 ("u16_mfma_wide"), on an 8-bit pair (q < 256 on
 *                       its u16 planes) and on a scaled-integer pair; any other pair: MIMC3_EUNSUPPORTED.  R beyond
 *                       mimc3_wide_planes_max_radius(ocw): MIMC3_EUNSUPPORTED, with the limit in the message.
 *   R >= 16, mode 0     an 8-bit pair goes where mimc3_match_ncc_wide_class (mode 0) sends it (last_path 14).  A scaled-integer pair runs
 *                       the u16-plane wide kernel (last_path 15) at every (ocw, R <= mimc3_wide_planes_max_radius(ocw)) named by the measured
 *                       rule below and at every such (ocw, R) mimc3_match_ncc_wide does not take; elsewhere mimc3_match_ncc_wide's kernel
 *                       where that takes (ocw, R) (last_path 10); beyond both kernels: MIMC3_EUNSUPPORTED.  Every other class is served
 *                       or refused as mimc3_match_ncc_wide_class does it.
 *   any other mode      MIMC3_EINVAL.  Every refusal comes before anything is enqueued or written, in the family's order.
 *   The kernel.  mimc3_match_ncc_full_chip_planes's (two 6-bit planes per pixel, three correlations per K chunk, sum ab put together in 64-bit
 *   integers, the row-box sums as three, four and one byte planes, the chip's sums in 64 x 64 sub-boxes of the packed u16 table, the null
 *   counts from the u32 null table, the f64 finish of the float kernel) over mimc3_match_ncc_wide_class's grid of ceil(S / 32)^2 tiles of
 *   32 x 32 cells: both chip planes staged once per point, both window tiles restaged per tile, the surface at pitch 96 in LDS bytes of its
 *   own, then mimc3_match_ncc_wide's tails, unmodified.  A clean form over all points flags those with a null in the chip or the box; a
 *   masked form runs behind it over the flagged points.
 *   Promise on an 8-bit or scaled-integer pair: record, candidates and surface are the bytes of the definition mimc3_match_ncc_wide states
 *   (mimc3_match_ncc_full_any in mode 1, word for word) -- at the six chip sizes within mimc3_wide_max_radius those of mimc3_match_ncc_wide
 *   itself (finite surface cells bit for bit, a non-finite cell of the same kind).
 *   mimc3_wide_planes_max_radius(ocw)   the largest R <= 47 whose layout -- two tiles, two chip planes, the surface of (2R + 1) x 96 x 4 bytes --
 *              fits the 160 KB of a CU: 47 for ocw 1..68; 46 / 45 / 44 / 43 at ocw 69 / 70 / 71 / 72; 34 at ocw 73, one less per ocw down to
 *              27 at ocw 80 (163,680 bytes); 0 outside 1..80.  The single source of the limit.
 *   mimc3_wide_planes_layout(ocw, R, out)   out[0] K chunks of 64 window columns per chip row (1..3), out[1] cell tiles per axis (2..3),
 *              out[2] threads per workgroup (128), out[3] dynamic LDS bytes, from the constexpr layout the launch uses; returns 1, or 0
 *              outside 1 <= ocw <= 80, 16 <= R <= mimc3_wide_planes_max_radius(ocw).
 *   The mode-0 rule: an (ocw, R) that mimc3_match_ncc_wide also takes goes to the matrix-core kernel where every pass of its series was
 *   faster than every pass of the float wide kernel's in the same session (tools/wide_u16_time.py, profiles/full_search_wide_u16/).
 *   Measured on C2 as 12-bit DN and as its d/dx pair (189,054 points, one MI355X): true in all 32 configurations the float kernel takes -- ocw 16 at
 *   R 16 / 23 / 31 / 32 / 47: 16.33 / 18.16 / 24.98 / 41.93 / 67.72 ms against 103.0 / 196.7 / 386.6 / 464.9 / 1296.0; ocw 7 at R 16 / 47: 7.78 / 38.58 against 19.9 / 276.3;
 *   ocw 40 at R 16: 151.7 against 1646.2 at R 16 -- and in a second run at ocw 15, 30 and 32 (R 16 and 47: 5.0 to 16.9 times faster), so every (ocw, R) that
 *   mimc3_match_ncc_wide takes goes to the matrix-core kernel; ocw 80, where it is the only kernel: 1170.5 / 1407.1 ms at R 16 / 27.
 *   MIMC3_hip_offsets calls this entry in mode 0 where it called mimc3_match_ncc_wide_class: the same files, a filtered pair and a 12-bit
 *   pair in a 16-bit TIFF on the matrix cores.
 *   Integral-f32 (16-bit DN) and float pairs beyond R 15 at any chip size: mimc3_match_ncc_wide_chip, below.
 *   Out of scope: mimc3_stack_add*, mimc3_match_ncc_wide_fb and Context.full_candidates through
 *   the class wide kernels; an ocw outside the six on the command line at R > 15; the pyramids; several GPUs. */
int mimc3_wide_planes_max_radius(int32_t ocw);
int mimc3_wide_planes_layout(int32_t ocw, int32_t R, int32_t out[4]);
int mimc3_match_ncc_wide_planes(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                                const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                                int32_t swap, int32_t mode, float *out /*[N][8] host*/,
                                float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_chip_planes_dev. */
int mimc3_match_ncc_wide_planes_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                    const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                    float *d_out, float *d_cand, float *d_surf, void *stream);

/* ---- The exhaustive search beyond +-15 px on ANY pair -- 16-bit DN (Landsat 8/9, Sentinel-2), float pixels (SAR amplitude), NaN or negative
 *      nulls -- at ANY chip half-width 1 <= ocw <= 80 (match_wide_chip_kernel.hip).
 *   The arguments are those of mimc3_match_ncc_wide_planes: 1 <= ocw <= 80, 1 <= R <= mimc3_wide_chip_max_radius(ocw) (47 in range, 0
 *   outside), npeaks 0..8, mode 0 or 1, surf optional; anything else MIMC3_EINVAL.  Every refusal comes before anything is enqueued or
 *   written, in the family's order.  In mode 0 the entry refuses no pair and no (ocw, R) in range.
 *                                  mode 0                                                      mode 1
 *   R <= 15                        mimc3_match_ncc_full_chip_planes(mode 0): its kernel,       mimc3_match_ncc_full_chip(mode 1)
 *                                  its bytes, its last_path                                    (last_path 11)
 *   R >= 16, 8-bit pair            where mimc3_match_ncc_wide_class(mode 0) sends it (14)      the kernel of this entry (16)
 *   R >= 16, scaled-integer pair   R <= mimc3_wide_planes_max_radius(ocw): where               16
 *                                  mimc3_match_ncc_wide_planes(mode 0) sends it (15);
 *                                  beyond: 16
 *   R >= 16, any other pair        ocw one of the six and R <= mimc3_wide_max_radius(ocw):     16
 *                                  mimc3_match_ncc_wide's kernel and bytes (10); else 16
 *   Definition (mode 1, and last_path 16 in mode 0): mimc3_match_ncc_full_any in mode 1, word for word, as mimc3_match_ncc_wide and
 *   mimc3_match_ncc_full_chip state it -- both null rules, f32 products widened to f64, additions only, the reference's f64 finish, the
 *   first-wins arg-max and the statuses -2 / -3 / -4, candidates by mimc3_match_ncc_wide's tail, the all-NaN record, candidates and
 *   surface for a point of the _dev entry that breaks the bounds.
 *   The kernel.  One workgroup of four wave64 per grid point.  The surface of S = 2R + 1 cells per side is ceil(S / 32)^2 tiles of 32 x 32
 *   cells (256 tasks of four cells, one per thread); per tile the chip is walked in bands of out[1] chip rows as
 *   mimc3_match_ncc_full_chip walks it: a band's chip rows and the h + 31 box rows they meet over the tile's window columns are staged,
 *   the band runs the clean or the masked body (a workgroup-uniform choice on the band's excluded pixels), the f64 accumulators stay in
 *   registers across the bands, the four cells are finished after the last band into a surface at pitch 96 with LDS bytes of its own.
 *   The validity counts (status -3) come from one pass over chip and box in front of the tiles.  Staging loads a pixel only if its BOX
 *   coordinates lie inside the (2R + 2 ocw + 1)^2 box: the overhang of a partial tile is staged as zeros, never read, never counted.
 *   The order of the additions is a function of (ocw, R) and of which body runs in which (tile, band), never of N, the point's place in the
 *   grid or timing; on 8-, 12- and 16-bit DN every sum is an exact integer and the bytes are those of the reference-order sums.
 *   mimc3_wide_chip_layout(ocw, R, out)   out[0] cell tiles per axis (2..3), out[1] chip rows per band, out[2] bands, out[3] workgroups
 *              per CU the LDS allows (at most 8), out[4] dynamic LDS bytes, from the constexpr layout the launch uses; returns 1, or 0
 *              outside 1 <= ocw <= 80, 16 <= R <= 47.  Two workgroups per CU wherever the whole chip is then one band; otherwise one
 *              workgroup and the tallest band that fits (ocw 80, R 47: 71 rows, three bands).
 *   mimc3_wide_chip_path(pair_class, ocw, R, mode)   the table above as a last_path number for a pair class (0 8-bit, 1 scaled-integer,
 *              2 integral f32, 3 any other); -1 outside the table.  No device.
 *   At the six chip sizes mode 0 keeps mimc3_match_ncc_wide's templated kernel: tools/wide_chip_time.py times the two side by side
 *   (profiles/full_search_wide_chip/, 18,906 of C2's points as 16-bit DN, one MI355X): ocw 16 at R 16 / 31 / 47: 29.70 / 34.77 / 77.12 ms
 *   against 11.1 / 40.5 / 136.6; ocw 40 at R 16 / 31: 350.4 / 349.0 against 172.2 / 352.5 -- faster with full tiles, 2.0 to 2.7 times slower at
 *   R 16, where three of the four tiles are nearly empty and cost full ones; ocw 80, where it is the only kernel: 1413.1 / 1385.5 / 3072.5.
 *   Not every pass is faster in every configuration, so nothing is moved.
 *   Out of scope: MIMC3_hip_offsets; forward-backward and mimc3_stack_add / _add_fused through this kernel; the pyramids beyond R 15;
 *   several GPUs; ocw above 80. */
int mimc3_wide_chip_max_radius(int32_t ocw);
int mimc3_wide_chip_layout(int32_t ocw, int32_t R, int32_t out[5]);
int mimc3_wide_chip_path(int32_t pair_class, int32_t ocw, int32_t R, int32_t mode);
int mimc3_match_ncc_wide_chip(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                              const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                              int32_t swap, int32_t mode, float *out /*[N][8] host*/,
                              float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, float *surf /*[N][(2R+1)^2] host, or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_wide_planes_dev. */
int mimc3_match_ncc_wide_chip_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                  const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                  float *d_out, float *d_cand, float *d_surf, void *stream);

/* ---- Forward-backward consistency of the exhaustive search: is a peak RECIPROCAL -- does matching back from where a point landed return
 *      to where it started?  (The back-matching test AMPCOR and IMCORR users apply after the run; the record's quality columns all
 *      describe one surface.)  One call: the forward search, then one backward search over the record and the candidates of every point,
 *      seeded on the device.
 *
 *   Forward pass   exactly mimc3_match_ncc_full_any(swap = 0, mode, surf = NULL) with the same arguments: out [N][8] and cand [npeaks][N][3]
 *                  are that call's bytes, on every pixel class; mimc3_ctx_last_path reports the forward path.
 *   Back-match of a forward result (du, dv) -- the record's columns 0, 1 for plane 0 of fb, candidate j's for plane 1 + j -- of grid point i:
 *     r  = ((int)rintf(du), (int)rintf(dv))          (f32, round half to even)
 *     m  = uv0 + offset + r                          (uv0 = ((int)xyuvav[i][2], (int)xyuvav[i][3]))
 *     the backward search is mimc3_match_ncc_full_any with swap = 1, the point's image coordinates replaced by m, offset' = -offset,
 *     shift' = -r, the same ocw, R and mode, npeaks = 0: the chip is cut from i1 at m, the search runs in i0 around m - offset - r = uv0.
 *     Its record is (du_b, dv_b, ncc_b, ...).
 *   Output fb, f32 [(1 + npeaks)][N][4], plane-major: the row is (du_b, dv_b, ncc_b, err),
 *     err = (float)hypot((double)du + (double)du_b, (double)dv + (double)dv_b): f64, rounded once; NaN unless du_b and dv_b are finite.
 *     A consistent match has d_b ~ -d_f: err near 0.
 *   Statuses, in column 2, with NaN in the other three columns:
 *     -5   the forward result has no fit (du or dv not finite: the record's status -2 / -3 / -4, an empty candidate slot, a NaN fit);
 *          nothing is searched;
 *     -6   the chip at m would leave the image (decided per point on the device; a fitted |du| or |dv| of 2^30 or more is this case
 *          too, without the conversion); nothing is searched.  The backward box itself always stays inside the 256-px zero border
 *          (it is centred on uv0, whose chip is inside the image, and R <= 15);
 *     -2 / -3 / -4   the backward search's own statuses pass through.
 *   With npeaks = 0 fb has one plane and cand is NULL.  Where the record has a fit, plane 1 (candidate 0) equals plane 0 bit for bit.
 *   Consequence: du_b, dv_b, ncc_b and the statuses equal bit for bit what a caller gets from two (with candidates 1 + npeaks) ordinary
 *   mimc3_match_ncc_full_any calls with the seed arithmetic above done on the host.  err is the device library's f64 hypot, which is
 *   accurate to an ulp of f64 but not documented as correctly rounded: against a host libm it can differ in the f32's last bit where the
 *   f64 value falls within an f64 ulp of an f32 rounding boundary (about one value in 2^28; exact cases -- a zero component, err = 0 --
 *   are exact on both sides).
 *   Refusals: those of mimc3_match_ncc_full_any (the host entry checks the FORWARD bounds only); fb NULL: MIMC3_EINVAL.
 *   Not covered: the pyramid entries, several GPUs, api.Context.full_candidates, any use of err inside the post-matcher chain. */
int mimc3_match_ncc_full_fb(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                            const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                            int32_t mode, float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                            float *fb /*[(1 + npeaks)][N][4] host*/);
/* Device-resident variant: the contract of mimc3_match_ncc_full_any_dev, plus d_fb [(1 + npeaks)][N][4].  Everything -- the forward
 * search, the seed, the backward search over (1 + npeaks) N rows, the composition -- is enqueued on `stream`, no sync.  The backward
 * rows, their records and one reason byte per row live in scratch of the context that grows on demand; all of it is sized before the
 * first launch, so only a call that makes it grow waits for the device, and it does so before it enqueues anything.  The caller's arrays
 * need no alignment beyond their element's: the two elementwise kernels read and write them element by element. */
int mimc3_match_ncc_full_fb_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t mode, float *d_out,
                                float *d_cand, float *d_fb, void *stream);
/* Forward-backward consistency beyond +-15 px: the text above under mimc3_match_ncc_wide's definition, 1 <= R <=
 * mimc3_wide_max_radius(ocw).  The forward pass is mimc3_match_ncc_wide(swap = 0, surf = NULL) -- out and cand are that call's bytes --
 * and the ONE backward pass over the (1 + npeaks) N seeded rows is mimc3_match_ncc_wide(swap = 1, offset' = -offset, shift' = -r,
 * npeaks = 0) on the same stream; seed, compose, err and the statuses -5 / -6 / -2 / -3 / -4 are as above.  R <= 15 returns the bytes of
 * mimc3_match_ncc_full_fb(mode 1).  mimc3_ctx_last_path reports the forward pass (10 at R >= 16, 9 below).  The backward box stays
 * inside the 256-px zero border: it is centred on uv0, which lies in the image, and R + ocw <= 79.  A wide box holds 9.4 times the
 * cells of a 31 x 31 one and as many more places for a decoy peak: err is the check that a peak found there is reciprocal.
 * Refusals: those of mimc3_match_ncc_wide (the host entry checks the FORWARD bounds only); fb NULL: MIMC3_EINVAL.
 * Not covered: as mimc3_match_ncc_full_fb. */
int mimc3_match_ncc_wide_fb(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                            const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t npeaks /*0 = record only*/,
                            float *out /*[N][8] host*/, float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/,
                            float *fb /*[(1 + npeaks)][N][4] host*/);
int mimc3_match_ncc_wide_fb_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, float *d_out, float *d_cand,
                                float *d_fb, void *stream);

/* ---- NCC stacking (ensemble matching; MIMC = Multiple Image, Multiple Chip): the correlation surfaces of several pairs that see the
 *      same motion -- a time series at equal separation, one pair at several chip sizes or after several filters; pairs of other
 *      separations through the scaled layers below -- are averaged cell by
 *      cell, and the peak is searched ONCE, on the mean surface.  Noise peaks do not repeat from layer to layer, the true peak does.
 *
 *   The stack is state of one context, and it outlives the pair: mimc3_ctx_set_images* and mimc3_ctx_filter_images do not touch it.
 *     N, R                   grid points and search radius; S = 2R + 1, cells in the surface's k order, k = (su + R) S + (sv + R)
 *     shift  i32 [N][2]      the search shift of every layer (all zero when none is given)
 *     sum    f64 [N][S^2]    cnt  u16 [N][S^2]    lay  u16 [N]    layers
 *   10 bytes per cell: 1.9 GB at 200,000 points and R 15.
 *
 *   Adding a layer -- a surface array surf [N][S^2] and a flag refused [N]:
 *     every cell v:   isfinite(v): sum += (double)v, cnt += 1;   any other cell (NaN, +-Inf) adds nothing;
 *     every point:    not refused: lay += 1;
 *     layers += 1.
 *   Additions happen in the order of the add calls; that order is part of the definition, so a result is deterministic and a host
 *   program that adds in f64 in the same order reproduces sum bit for bit.
 *   Mean surface at min_count >= 1:  mean[k] = (float)(sum[k] / (double)cnt[k]) where cnt[k] >= min_count, NaN elsewhere (the division
 *   is f64, rounded once to f32).
 *   Result:  a point with lay == 0 gets status -3 in its record and in every candidate slot.  Any other point gets exactly what the
 *   tail of the exhaustive search makes of mean with the stack's shift: the record of mimc3_match_ncc_full_any -- statuses -2 (no
 *   finite cell) and -4 (peak on the border), the 3x3 fit, ncc_fit, SNR, the Hessian -- and the npeaks <= 8 ranked local maxima.
 *   du, dv are relative to uv0 + offset, as everywhere; offset may differ from layer to layer (it is each pair's co-registration),
 *   shift, N and R are the stack's.
 *   Consequence: a stack of ONE layer at min_count 1 returns the record and the candidates of mimc3_match_ncc_full_any(mode 1) bit for
 *   bit, because (float)((double)v / 1.0) == v.
 *   Beyond R 15 (mimc3_stack_begin_wide, 16 <= R <= 47): the same state, layout and definition; a layer from the resident pair is
 *   mimc3_match_ncc_wide's surface, and the tail is that entry's (one workgroup per point, the candidates from up to 95 x 95 cells), so
 *   a stack of ONE layer returns the bytes of mimc3_match_ncc_wide.  The state is 10 bytes per cell whatever R is: 18 GB at 200,000
 *   points and R 47.
 *   Not covered: several GPUs, the pyramid entries, MIMC3_hip_offsets.  (These entries write a layer beyond R 15, and every scaled
 *   layer, to the layer scratch and read it back once; mimc3_stack_add_fused and mimc3_stack_add_scaled_fused do not.)
 *
 *   Layers of another time baseline: scaled and weighted (mimc3_stack_add_scaled, mimc3_stack_add_surfaces_scaled).  Pairs of different
 *   separation share a velocity, not a displacement: what moved d px in the stack's interval moved s d px in a pair s times as long.
 *   A scaled layer has
 *     a scale s (f64: the layer's time separation over the stack's), finite, 2^-6 <= s <= 2^6;
 *     a weight w (f64), finite, > 0;
 *     a layer radius Rl, Sl = 2 Rl + 1;
 *     surfaces L [N][Sl^2] in k order, k = ju Sl + jv, ju, jv in 0..2 Rl;   a flag refused [N].
 *   The layer was searched around the layer shift, once per point:
 *     Lsh[i] = ((int32)rint(s * (double)shift[i][0]), (int32)rint(s * (double)shift[i][1]))
 *   -- the product is f64, rint rounds half to even; |s * shift| >= 2^30 is refused with MIMC3_EINVAL by every entry (the context keeps a
 *   host copy of the shift).  Every operation below is a single f64 operation, rounded, in the order written (the library is built
 *   with -ffp-contract=off: nothing fuses).  For stack cell (su, sv) in [-R, R]^2 of point i:
 *     pu = s * (double)(shift[i][0] + su) - (double)Lsh[i][0]      fu = floor(pu)   au = pu - fu   ju = (int)fu + Rl
 *     pv = s * (double)(shift[i][1] + sv) - (double)Lsh[i][1]      fv = floor(pv)   av = pv - fv   jv = (int)fv + Rl
 *     row(j) = av == 0 ? (double)L[j][jv]  : (1 - av) * (double)L[j][jv] + av * (double)L[j][jv + 1]
 *     value  = au == 0 ? row(ju)           : (1 - au) * row(ju)          + au * row(ju + 1)
 *   A tap with weight zero is NOT read: at au == 0 the row ju + 1 is not read, at av == 0 the column jv + 1 is not read; such a tap
 *   may be NaN or lie outside the layer.  The cell is finite when every tap that is read lies inside 0..2 Rl on both axes and value is
 *   finite.
 *     a finite cell:   sum += w * value (one product, one addition), cnt += 1, wsum += w;   any other cell adds nothing;
 *     every point:     not refused: lay += 1;
 *     layers += 1.
 *   The order of the adds is part of the definition, as above.
 *   wsum is a third per-cell plane, f64 [N][S^2], and it exists only on a WEIGHTED stack: the first add whose w != 1.0 allocates it and
 *   initialises it to (double)cnt (one elementwise kernel, enqueued on that add's stream before the add); from then on every add of
 *   either kind maintains it -- mimc3_stack_add and mimc3_stack_add_surfaces add 1.0.  mimc3_stack_begin* and the release forget it.
 *   Mean surface:  (float)(sum / wsum) on a weighted stack, (float)(sum / (double)cnt) otherwise; where cnt >= min_count, NaN elsewhere.
 *   The state is 10 bytes per cell until the first weighted add, then 18.
 *   Consequences:
 *     s == 1, w == 1, Rl == R:  pu, pv are integers ((double)(shift + su) - (double)shift is exact), every cell is one tap, value ==
 *       (double)v, and the stack's bytes are those of mimc3_stack_add / mimc3_stack_add_surfaces.
 *     every layer at the same power-of-two weight:  sum and wsum are the unweighted sum and cnt times that power, exactly, and the mean
 *       is the unweighted mean bit for bit.
 *   Not covered by the scaled layers: several GPUs, the pyramid entries, forward-backward, MIMC3_hip_offsets.  (Fusing the accumulation
 *   into the search: mimc3_stack_add_scaled_fused, on 8-bit and scaled-integer pairs.) */
#define MIMC3_STACK_CHUNK 65536
/* Sizes and zeroes the stack and uploads shift (host [N][2], or NULL).  1 <= R <= 15.  A second call discards the first stack; N = 0
 * releases its memory (R and shift are then ignored).  A chip-atlas context: MIMC3_ESTATE.  Returns when the stack is ready. */
int mimc3_stack_begin(mimc3_ctx *ctx, int32_t N, int32_t R, const int32_t *shift /*host [N][2] or NULL*/);
/* mimc3_stack_begin with 1 <= R <= 47 (the largest mimc3_wide_max_radius).  With R <= 15 it leaves the context exactly as
 * mimc3_stack_begin does.  On a stack of R >= 16: mimc3_stack_add / _add_dev take a layer that is mimc3_match_ncc_wide(npeaks 0, shift =
 * the stack's, surf) on the resident pair, and refuse an ocw with R > mimc3_wide_max_radius(ocw) (ocw 40 on a stack of R 40..47) with
 * MIMC3_EINVAL, before anything is enqueued; points go in chunks of mimc3_stack_chunk(R); mimc3_stack_add_surfaces takes S^2 up to 9,025
 * cells per point; mimc3_stack_finish runs the tail of mimc3_match_ncc_wide. */
int mimc3_stack_begin_wide(mimc3_ctx *ctx, int32_t N, int32_t R, const int32_t *shift /*host [N][2] or NULL*/);
/* The points of one accumulation launch at radius R: MIMC3_STACK_CHUNK for 1 <= R <= 15, floor(MIMC3_STACK_CHUNK 961 / (2R+1)^2) for
 * 16 <= R <= 47 (57,832 at R 16, 6,978 at R 47: the layer scratch never exceeds the 252 MB of R 15), 0 for any other R. */
int32_t mimc3_stack_chunk(int32_t R);
/* One layer from the resident pair: mimc3_match_ncc_full_any(mode 1, npeaks 0, shift = the stack's, surf) with these arguments; a point
 * is refused where that call's record has status -3.  Points go in chunks of MIMC3_STACK_CHUNK through a layer scratch of the context
 * (a buffer of its own, at most 252 MB whatever N is).  Refusals: those of mimc3_match_ncc_full_any; N differs from the stack's:
 * MIMC3_EINVAL; no stack: MIMC3_ESTATE; 65,535 layers added: MIMC3_ESTATE.  Everything is validated before the first launch: a refused
 * add leaves the stack's bytes as they were. */
int mimc3_stack_add(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap);
/* Device-resident variant: everything is enqueued on `stream`, no sync (the first call on a pair builds its f32 planes on the context's
 * own stream and waits for them first; a call that makes the layer scratch grow waits for the device before it enqueues anything).  A
 * point that breaks the host entry's bounds has an all-NaN surface and counts as a layer (the contract of the _dev search entries). */
int mimc3_stack_add_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t swap,
                        void *stream);
/* mimc3_stack_add through the kernel of the pair's class: its arguments and its refusals.  On a stack of R <= 15 the layer is
 * mimc3_match_ncc_full_surf(npeaks 0, shift = the stack's, surf) -- the same chunks of mimc3_stack_chunk(R) points through the same layer
 * scratch and the same accumulation -- so an 8-bit, 12-bit or 16-bit DN layer costs its own kernel's search and not the float kernel's.
 * The accumulation adds only finite cells and takes the refused points from the record's status -3, and the class kernel's finite
 * cells and records are the float kernel's bit for bit (see mimc3_match_ncc_full_surf): the stack's state after this call -- sum, cnt,
 * lay, wsum -- is bit for bit the state after mimc3_stack_add, on every pixel class, and the two may be mixed freely.  A weighted
 * stack's wsum gets 1.0 per finite cell, as from mimc3_stack_add.  On a stack of R >= 16 the call IS mimc3_stack_add (the wide kernel),
 * byte for byte: a caller does not have to branch.  mimc3_ctx_last_path reports the kernel that ran (6 / 7 / 8 / 9; 10 beyond R 15).
 * Not covered: scaled layers through the templated class kernels; the layer scratch round trip stays here (mimc3_stack_add_fused and
 * mimc3_stack_add_scaled_fused below fuse the accumulation into the run-time-ocw matrix-core searches). */
int mimc3_stack_add_class(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap);
/* Device-resident variant, under the contract of mimc3_stack_add_dev (a first call on a pair builds the planes and tables its kernel
 * reads on the context's own stream and waits for them first). */
int mimc3_stack_add_class_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t swap,
                              void *stream);
/* One layer from the resident pair at ANY chip half-width 1 <= ocw <= 80 and any stack radius, accumulated in the search's own tail.
 *   Definition: the layer is mimc3_match_ncc_wide_planes(mode 0, npeaks 0, shift = the stack's, R = the stack's, surf) on the resident
 *   pair (at R <= 15 that is mimc3_match_ncc_full_chip_planes), added as mimc3_stack_add_surfaces adds it with the refused points taken
 *   from the record (status -3).  The stack's state afterwards -- sum, cnt, lay, wsum -- is bit for bit the state after that two-call
 *   chain; at the six chip sizes 7, 15, 16, 30, 32, 40 it is the state after mimc3_stack_add / mimc3_stack_add_class as well, and all
 *   the adds may be mixed freely.  A weighted stack's wsum gets 1.0 per finite cell.
 *   Which kernel runs (mimc3_ctx_last_path reports it after every add):
 *     8-bit pair       12 ("u8_mfma_chip") at R <= 15, 14 ("u8_mfma_wide") at 16 <= R <= 47, at every ocw 1..80, the six included --
 *                      the ACCUMULATING forms of the run-time-ocw matrix-core kernels: every workgroup adds the finished surface of its
 *                      point into the stack from LDS (one lane owns a cell: plain read-modify-writes), no tail runs, and no record,
 *                      candidate or surface is written.  One launch pair over all N points: no layer scratch, no record scratch, no chunks.
 *     scaled-integer   13 ("u16_mfma_chip") at R <= 15, 15 ("u16_mfma_wide") up to mimc3_wide_planes_max_radius(ocw), the same way
 *                      (12-bit DN, the pair after mimc3_ctx_filter_images).
 *     any other pair   (16-bit DN, floats) not fused: the kernel mimc3_match_ncc_wide_planes(mode 0, surf) runs (8 / 9 at the six and
 *                      11 elsewhere up to R 15, 10 beyond at the six) through the layer scratch and the accumulation of mimc3_stack_add in
 *                      chunks of mimc3_stack_chunk(R); where no kernel takes (ocw, R) the call is refused.
 *   mimc3_stack_fused_max_radius(ctx, ocw): the largest stack radius this entry takes for the resident pair's class at that ocw -- 47
 *   on an 8-bit pair, mimc3_wide_planes_max_radius(ocw) on a scaled-integer one, else 15, or mimc3_wide_max_radius(ocw) at the six; 0
 *   for an ocw outside 1..80, without images and on a chip-atlas context.  (On a pair that is neither 8-bit nor scaled-integer the
 *   first query builds the pair's f32 planes, as a search would.)
 *   Refusals, all before anything is allocated, enqueued or counted (the stack and mimc3_stack_info stay as they were): ocw outside
 *   1..80, a null pointer, N <= 0: MIMC3_EINVAL; no images, a chip-atlas context: MIMC3_ESTATE; the stack's own, as every add words them
 *   (no stack, 65,535 layers: MIMC3_ESTATE; N differs: MIMC3_EINVAL); a stack radius beyond mimc3_stack_fused_max_radius(ctx, ocw):
 *   MIMC3_EINVAL, with the limit in the message; the host entry: a chip that leaves the image, a search box that leaves the zero border:
 *   MIMC3_EBOUNDS.
 *   Not covered: the pyramids, several GPUs, 16-bit kernels at other chip sizes (scaled layers through these kernels:
 *   mimc3_stack_add_scaled_fused below). */
int mimc3_stack_add_fused(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t swap);
/* Device-resident variant, under the contract of mimc3_stack_add_dev: a point that breaks the host entry's bounds adds no cell and
 * counts as a layer (a first call on a pair builds the planes and tables its kernel reads on the context's own stream and waits for them). */
int mimc3_stack_add_fused_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw, int32_t swap,
                              void *stream);
int32_t mimc3_stack_fused_max_radius(mimc3_ctx *ctx, int32_t ocw);
/* One layer from the caller's surfaces -- of another context, of a later kernel, crafted: surf [N][S^2] in k order, refused [N]
 * (not 0 = refused) or NULL (no point is).  Refusals: the stack's, as above. */
int mimc3_stack_add_surfaces(mimc3_ctx *ctx, const float *surf /*host [N][S^2]*/, const uint8_t *refused /*host [N] or NULL*/, int32_t N);
int mimc3_stack_add_surfaces_dev(mimc3_ctx *ctx, const float *d_surf, const uint8_t *d_refused, int32_t N, void *stream);
/* The result.  out [N][8]; cand [npeaks][N][3], NULL iff npeaks == 0 (npeaks 0..8); surf [N][S^2] gets mean and count [N] gets lay
 * when given.  Reads the stack and leaves it unchanged: more layers may follow, and finishing twice gives the same bytes.
 * min_count < 1 or > 65535: MIMC3_EINVAL; no stack: MIMC3_ESTATE. */
int mimc3_stack_finish(mimc3_ctx *ctx, int32_t npeaks, int32_t min_count, float *out /*[N][8] host*/,
                       float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, float *surf /*[N][S^2] host, or NULL*/,
                       uint16_t *count /*[N] host, or NULL*/);
int mimc3_stack_finish_dev(mimc3_ctx *ctx, int32_t npeaks, int32_t min_count, float *d_out, float *d_cand, float *d_surf,
                           uint16_t *d_count, void *stream);
/* N, R and the number of layers added (each may be NULL); all 0 when the context has no stack. */
int mimc3_stack_info(mimc3_ctx *ctx, int32_t *N, int32_t *R, int32_t *layers);
/* The smallest layer radius that serves every cell of a stack of radius R at this scale, whatever the shift: R when scale == 1, else
 * (int32_t)floor(scale R + 0.5) + 1 -- a stack cell su lands at pu = s su + (s sh - rint(s sh)), and |s sh - rint(s sh)| <= 0.5, so
 * |pu| <= s R + 0.5 and the taps floor(pu), floor(pu) + 1 lie within floor(s R + 0.5) + 1 of the layer's centre.  0 for R outside 1..47
 * or a scale outside 2^-6..2^6.  The result may exceed 47 (or mimc3_wide_max_radius(ocw)): the caller then passes a smaller layer_R, and
 * the outer cells of the stack get no count from that layer -- count, cnt and min_count express that. */
int32_t mimc3_stack_layer_radius(int32_t R, double scale);
/* Lsh of the definition, from the stack's host shift.  No stack: MIMC3_ESTATE; a bad scale or |scale shift| >= 2^30: MIMC3_EINVAL. */
int mimc3_stack_layer_shift(mimc3_ctx *ctx, double scale, int32_t *out /*host [N][2]*/);
/* 1 when the context's stack is weighted (it has a wsum plane), else 0. */
int mimc3_stack_weighted(mimc3_ctx *ctx);
/* One scaled layer from the resident pair: mimc3_match_ncc_wide(npeaks 0, shift = Lsh, R = layer_R, surf) with these arguments (the
 * float kernel up to layer_R 15, the wide kernel beyond), resampled into the stack by the definition above; a point is refused where
 * that call's record has status -3.  1 <= layer_R <= mimc3_wide_max_radius(ocw), whatever the stack's R (1..47, begun by either
 * mimc3_stack_begin or _begin_wide).  Points go in chunks of min(mimc3_stack_chunk(R), mimc3_stack_chunk(layer_R)) through the layer
 * scratch.  The host entry checks the chips and the layer's box (layer_R + ocw around uv0 + offset + Lsh) against the zero border as
 * mimc3_stack_add does: MIMC3_EBOUNDS.  A bad scale, weight or layer_R, |scale shift| >= 2^30, N differs: MIMC3_EINVAL; no stack, no
 * images, 65,535 layers: MIMC3_ESTATE.  Everything is validated before the first launch or allocation that touches the stack: a refused
 * add leaves the stack's bytes, and whether it is weighted, as they were. */
int mimc3_stack_add_scaled(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t layer_R,
                           int32_t swap, double scale, double weight);
/* Device-resident variant, under the contract of mimc3_stack_add_dev. */
int mimc3_stack_add_scaled_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                               int32_t layer_R, int32_t swap, double scale, double weight, void *stream);
/* mimc3_stack_add_scaled at ANY chip half-width 1 <= ocw <= 80 and any layer radius the pair's class reaches, resampled in the search's
 * own tail.
 *   Definition: the layer is mimc3_match_ncc_wide_planes(mode 0, npeaks 0, shift = Lsh, R = layer_R, surf) on the resident pair (at
 *   layer_R <= 15 that is mimc3_match_ncc_full_chip_planes), Lsh the layer shift of the definition above, added as
 *   mimc3_stack_add_surfaces_scaled(surf, refused, layer_R, scale, weight) adds it with the refused points taken from the record (status
 *   -3).  The stack's state afterwards -- sum, cnt, lay, wsum, and whether it is weighted -- is bit for bit the state after that
 *   two-call chain; at the six chip sizes with layer_R <= mimc3_wide_max_radius(ocw) it is the state after mimc3_stack_add_scaled as
 *   well; scale 1, weight 1, layer_R = R gives the bytes of mimc3_stack_add_fused; every kind of add may be mixed with every other.
 *   Limits: 1 <= ocw <= 80; 1 <= layer_R <= mimc3_stack_fused_max_radius(ctx, ocw), whatever the stack's R (1..47, begun by either
 *   mimc3_stack_begin or _begin_wide): the stack's radius and the layer's are independent.
 *   Which kernel runs (mimc3_ctx_last_path reports it after every add), chosen by layer_R:
 *     8-bit pair       12 ("u8_mfma_chip") at layer_R <= 15, 14 ("u8_mfma_wide") beyond -- the accumulating forms of mimc3_stack_add_fused,
 *                      which here RESAMPLE: after the barrier that completes a point's layer surface in LDS the workgroup walks the
 *                      STACK's cells, and each takes its bilinear value from the surface by the definition above, operation for
 *                      operation (one lane owns a stack cell: plain read-modify-writes).  One launch pair over all N points: no layer
 *                      scratch, no record scratch, no chunks, no LDS beyond the search's own.
 *     scaled-integer   13 ("u16_mfma_chip") / 15 ("u16_mfma_wide"), the same way (12-bit DN, the pair after mimc3_ctx_filter_images).
 *     any other pair   (16-bit DN, floats) not fused: the kernel mimc3_match_ncc_wide_planes(mode 0, surf) runs (8 / 9 at the six and 11
 *                      elsewhere up to layer_R 15, 10 beyond at the six) through the layer scratch and the accumulation of
 *                      mimc3_stack_add_scaled in chunks of min(mimc3_stack_chunk(R), mimc3_stack_chunk(layer_R)) -- which gives those
 *                      pairs scaled layers at every chip size up to layer_R 15; where no kernel takes (ocw, layer_R) the call is refused.
 *   Before the launch, on the call's stream, what every scaled add enqueues: the wsum plane of a stack that this add makes weighted
 *   (the first weight != 1.0), and the layer shift.
 *   Refusals, all before anything is allocated, enqueued or counted (the stack's bytes, mimc3_stack_info and mimc3_stack_weighted stay
 *   as they were): those of mimc3_stack_add_fused (ocw outside 1..80, a null pointer, N <= 0: MIMC3_EINVAL; no images, a chip-atlas
 *   context: MIMC3_ESTATE; no stack, 65,535 layers: MIMC3_ESTATE; N differs: MIMC3_EINVAL); a scale outside 2^-6..2^6, a weight that is
 *   not finite and > 0, a layer_R outside 1..mimc3_stack_fused_max_radius(ctx, ocw) (the limit is in the message), |scale shift| >=
 *   2^30: MIMC3_EINVAL; the host entry: a chip that leaves the image, the LAYER's box (layer_R + ocw around uv0 + offset + Lsh) that
 *   leaves the zero border: MIMC3_EBOUNDS.
 *   Not covered: mimc3_stack_add_surfaces_scaled is unchanged (a caller's surfaces go through stack_add_scaled_kernel); 16-bit pairs
 *   beyond layer_R 15 at chip sizes outside the six; the pyramids; several GPUs; MIMC3_hip_offsets. */
int mimc3_stack_add_scaled_fused(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2], int32_t ocw, int32_t layer_R,
                                 int32_t swap, double scale, double weight);
/* Device-resident variant, under the contract of mimc3_stack_add_dev: a point that breaks the host entry's bounds adds no cell and
 * counts as a layer. */
int mimc3_stack_add_scaled_fused_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, int32_t ocw,
                                     int32_t layer_R, int32_t swap, double scale, double weight, void *stream);
/* One scaled layer from the caller's surfaces, which the caller searched around mimc3_stack_layer_shift: surf [N][Sl^2] in k order,
 * 1 <= layer_R <= 47, refused [N] or NULL.  Refusals: as above, without those of the search. */
int mimc3_stack_add_surfaces_scaled(mimc3_ctx *ctx, const float *surf /*host [N][Sl^2]*/, const uint8_t *refused /*host [N] or NULL*/,
                                    int32_t N, int32_t layer_R, double scale, double weight);
int mimc3_stack_add_surfaces_scaled_dev(mimc3_ctx *ctx, const float *d_surf, const uint8_t *d_refused, int32_t N, int32_t layer_R,
                                        double scale, double weight, void *stream);

/* ---- Coarse-to-fine exhaustive search over an image pyramid (no reference counterpart: the reach of mimc3_match_ncc_full, +-R
 *      around uv0 + offset + shift, made about R (2^L - 1) px by searching a reduced pair first -- the offset trackers' standard).
 *
 *   Inputs: those of mimc3_match_ncc_full, plus levels L, 1 <= L <= 5; the pair must be 8-bit (u8 planes).  For grid point i:
 *     starting displacement  (u0, v0) = ((int)xyuvav[i][2], (int)xyuvav[i][3]);  D = offset + shift[i] (shift NULL = zero).
 *     levels     level 0 is the resident pair; level l has H_l = H_{l-1} >> 1, W_l = W_{l-1} >> 1 (an odd last row or column is
 *                dropped), and its pixel (x, y) comes from the 2 x 2 block I_{l-1}[2y..2y+1][2x..2x+1]: with n the number of its
 *                non-zero (non-null) pixels and s their sum, (s + n/2) / n in integer arithmetic (nearest, ties up), or 0 when n = 0.
 *                A level pixel stays in 0..255 and is null exactly when its whole block is.  The point sits at p_l = (u0 >> l, v0 >> l).
 *     coarsest   d_{L-1} = floor((D + 2^{L-2}) / 2^{L-1}) per axis (arithmetic shift); for L = 1, d_0 = D.
 *     l = L-1 .. 1  the exhaustive search of mimc3_match_ncc_full on the level-l pair at p_l, with offset 0, shift d_l and the same
 *                ocw, R and swap (its validity and first-wins arg-max rules unchanged).  If it has an arg-max cell (su, sv) -- a peak
 *                on the border (status -4) included: it still points the way -- d_{l-1} = 2 (d_l + (su, sv)); otherwise (status -3,
 *                -2, a chip that leaves the level image, a search box beyond the level planes' 256-px zero border) d_{l-1} = 2 d_l.
 *     level 0    the [N][8] record of the exhaustive search at uv0 with the caller's offset and shift_out[i] = d_0 - offset: bit for
 *                bit what mimc3_match_ncc_full(ctx, xyuvav, N, offset, shift_out, ocw, R, swap) returns wherever that call accepts
 *                the input.  A point whose derived level-0 search box leaves the 256-px zero border gets the all-NaN record (the
 *                _dev entry's contract); the call is not refused.
 *   Output: out [N][8] as mimc3_match_ncc_full; shift_out [N][2] (optional): d_0 - offset, the shift of the level-0 search.
 *   Refusals: levels outside 1..5, a level-(L-1) image smaller than a chip (min(H_{L-1}, W_{L-1}) < 2 ocw + 1), a starting
 *   displacement (offset, or offset + shift[i]) beyond +-2^24 on an axis, and every refusal of mimc3_match_ncc_full for ocw and R:
 *   MIMC3_EINVAL; a chip that leaves the level-0 image: MIMC3_EBOUNDS; a pair that is not 8-bit: MIMC3_EUNSUPPORTED.
 *   mimc3_ctx_last_path reports 6.  The levels are built on the first call that needs them and kept until the pair changes; all L
 *   searches and the steps between them run on one stream, with no host round trip between levels. */
int mimc3_match_ncc_pyramid(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                            const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t levels, int32_t swap,
                            float *out /*[N][8] host*/, int32_t *shift_out /*[N][2] host or NULL*/);
/* Device-resident variant: d_xyuvav [N][6], d_shift [N][2] or NULL, d_out [N][8], d_shift_out [N][2] or NULL device pointers;
 * enqueues on `stream`, no sync (a first call on a pair builds its levels on the context's stream and drains it first).  The caller
 * guarantees the chip and displacement bounds the host entry checks. */
int mimc3_match_ncc_pyramid_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t swap,
                                float *d_out, int32_t *d_shift_out /*or NULL*/, void *stream);
/* ---- Coarse-to-fine exhaustive search on every pair mimc3_match_ncc_full_dn takes: 8-bit, scaled-integer (12-bit DN, a filtered 8-bit
 *      pair) and integral-f32 pairs (16-bit DN -- Landsat 8/9 OLI, Sentinel-2 -- and its filtered forms), with candidates at level 0.
 *
 *   mimc3_match_ncc_pyramid's definition word for word -- levels 1..5, p_l = (u0 >> l, v0 >> l), d_{L-1} = floor((D + 2^{L-2}) / 2^{L-1}),
 *   d_{l-1} = 2 (d_l + s) with the level's arg-max cell s or 2 d_l without one, shift_out = d_0 - offset, the +-2^24 bound on the starting
 *   displacement, the refusal of a coarsest level smaller than a chip, the all-NaN record for a level-0 box beyond the zero border, one
 *   stream and no host round trip -- with three things new:
 *   Classes.  The pair the context currently matches on is classified once, as by mimc3_match_ncc_full_dn; the class of level 0 decides
 *     the kernels of every level, and a level is never classified again:
 *       8-bit pair       the u8 levels and matrix-core kernels of mimc3_match_ncc_pyramid.  mimc3_ctx_last_path reports 6.  With npeaks = 0,
 *                        record and shift_out are mimc3_match_ncc_pyramid's bit for bit.
 *       scaled-integer   u16 levels, the kernels of mimc3_match_ncc_full_planes.  mimc3_ctx_last_path reports 7.
 *       integral f32     f32 levels with 16-byte tables, the kernels of mimc3_match_ncc_full_dn.  mimc3_ctx_last_path reports 8.
 *       anything else    (non-integral data, NaN nulls, values of 2^20 and above) MIMC3_EUNSUPPORTED.  (mimc3_match_ncc_pyramid_any takes it.)
 *   Reduction, on integers.  With w = pixel * 2^s, s the image's shift (0 or 3: the one its class was established with), a level pixel is
 *     ((sum w + n/2) / n) / 2^s in integer arithmetic over the n non-zero pixels of its 2 x 2 block, or 0 when n = 0; H >> 1 x W >> 1 (an odd
 *     last row or column is dropped); the level inherits the shift.  Both classes are closed under the rule (a mean of values below 4096
 *     stays below 4096, one of values below 2^20 below 2^20; the sum stays below 2^22), and a pixel is null exactly when its whole block
 *     is.  On an 8-bit pair s = 0 and this is mimc3_match_ncc_pyramid's reduction.
 *     The levels are reductions of the planes the context CURRENTLY matches on: after mimc3_ctx_filter_images that is the filtered pair.
 *     The rule is filter, then reduce -- not the filter of the reduced pair.
 *   Candidates.  npeaks in 0..8, cand [npeaks][N][3] with npeaks > 0 (NULL with 0), as mimc3_match_ncc_full_dn.  Level 0 IS
 *     mimc3_match_ncc_full_dn with shift = shift_out, its candidates included (on an 8-bit pair: mimc3_match_ncc_full_multi's kernels);
 *     the coarser levels never compute candidates.  A point that gets the all-NaN record gets all-NaN candidate slots.
 *   Refusals: those of mimc3_match_ncc_pyramid, with the class rule above in place of "not 8-bit"; npeaks outside 0..8, or cand NULL with
 *   npeaks > 0 / not NULL with npeaks = 0: MIMC3_EINVAL.
 *   Not covered: several devices, a candidates-over-variants driver of its own (api.Context.full_candidates(levels) goes through mimc3_match_ncc_pyramid_chip). */
int mimc3_match_ncc_pyramid_dn(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                               const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t levels,
                               int32_t npeaks /*0 = record only*/, int32_t swap, float *out /*[N][8] host*/,
                               float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, int32_t *shift_out /*[N][2] host or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_pyramid_dev, plus d_cand [npeaks][N][3] (NULL iff npeaks == 0). */
int mimc3_match_ncc_pyramid_dn_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                   const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap,
                                   float *d_out, float *d_cand, int32_t *d_shift_out /*or NULL*/, void *stream);
/* ---- Coarse-to-fine exhaustive search on ANY f32 pair: the pairs of mimc3_match_ncc_full_any (non-integral pixels, NaN or negative
 *      nulls), which need the reach most.  The arguments of mimc3_match_ncc_pyramid_dn plus `mode` (after swap, as in
 *      mimc3_match_ncc_full_any); there is no surf argument.
 *
 *   mimc3_match_ncc_pyramid's definition word for word -- levels 1..5, p_l = (u0 >> l, v0 >> l), d_{L-1} = floor((D + 2^{L-2}) / 2^{L-1}),
 *   d_{l-1} = 2 (d_l + s) with the level's arg-max cell s (a status -4 peak counts) or 2 d_l without one, shift_out = d_0 - offset, the
 *   +-2^24 bound on the starting displacement, the refusal of a coarsest level smaller than a chip, the all-NaN record (and all-NaN
 *   candidate slots) for a level-0 box beyond the 256-px zero border, one stream and no host round trip, the same refusals -- with:
 *   mode 0   on an 8-bit, scaled-integer or integral-f32 pair: exactly mimc3_match_ncc_pyramid_dn -- its levels, its kernels, its bytes;
 *            mimc3_ctx_last_path reports 6 / 7 / 8.  On every other f32 pair: the float levels and the float kernel below;
 *            mimc3_ctx_last_path reports 9.
 *   mode 1   the float levels and the float kernel on any pair, whatever its class (built beside that class's own levels; both sets
 *            stay valid until the pair changes).
 *   Any other mode: MIMC3_EINVAL.  Class is no reason to refuse.
 *   Float reduction.  Level l has H_{l-1} >> 1 x W_{l-1} >> 1 pixels (an odd last row or column is dropped).  A pixel p of the 2 x 2 block
 *     is INCLUDED when (double)p >= 1e-10 -- the reference's inclusion rule: NaN, 0, -0.0, negatives and positives below MIN_DN are not.
 *     With n the number of included pixels and S their f64 sum, added in the fixed order (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1),
 *     the level pixel is (float)(S / (double)n), or 0.0f when n = 0.  (The order is fixed so that the reduction can be restated bit for
 *     bit.)  An included +Inf goes through the arithmetic: the pixel is +Inf.
 *     A block with no included pixel becomes the canonical null 0 -- an all-NaN block too.  So on a coarser level an area that is all
 *     no-data, in whatever encoding, counts under the validity rule and is refused with status -3, where on level 0 an all-NaN chip is
 *     "valid, no cell" (-2).  This is deliberate: a coarser level only steers the search, and a chip that is mostly no-data must not
 *     steer it.
 *     Level 0 is the zero-bordered f32 plane pair as it stands; the levels are reductions of the pair the context CURRENTLY matches on
 *     (after mimc3_ctx_filter_images: filter, then reduce).  No tables are built for these levels.
 *   Searches.  Levels L-1 .. 1 are the exhaustive search of mimc3_match_ncc_full_any in mode 1 on the level pair -- its two null rules,
 *     its terms, its finish -- in the summation order that entry uses for npeaks == 0.  Level 0 IS mimc3_match_ncc_full_any with the
 *     caller's mode at shift = shift_out, candidates included.  Consequence: on the float class, record and shift_out equal bit for bit
 *     what a caller gets by chaining mimc3_match_ncc_full_any(mode 1, surf) over the same levels by hand (arg-max of surf: the lowest k
 *     among the largest finite cells).  On an integer-class pair whose float and integer levels coincide, mode 1 returns the bytes of
 *     mimc3_match_ncc_pyramid_dn.
 *   Refusals: those of mimc3_match_ncc_pyramid_dn without its class rule; mode outside 0..1: MIMC3_EINVAL.
 *   Not covered: several GPUs; a candidates-over-variants driver of its own (api.Context.full_candidates(levels) goes through mimc3_match_ncc_pyramid_chip); MIMC3_hip_offsets
 *   on float TIFFs. */
int mimc3_match_ncc_pyramid_any(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                                const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t levels,
                                int32_t npeaks /*0 = record only*/, int32_t swap, int32_t mode, float *out /*[N][8] host*/,
                                float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, int32_t *shift_out /*[N][2] host or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_pyramid_dn_dev.  (The first call on a pair builds its f32 planes and float
 * levels on the context's own stream and waits for them before it enqueues on `stream`.) */
int mimc3_match_ncc_pyramid_any_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                    const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap,
                                    int32_t mode, float *d_out, float *d_cand, int32_t *d_shift_out /*or NULL*/, void *stream);
/* ---- Coarse-to-fine exhaustive search at ANY chip half-width 1 <= ocw <= mimc3_full_chip_max_ocw() (80), on the run-time-ocw kernels:
 *      the reference's chip sets 7/10/15, 11/14 and 30/60/80 coarse to fine, and the 8-bit, 12-bit and filtered pairs on the matrix
 *      cores on every level.  The arguments of mimc3_match_ncc_pyramid_any.  R 1..15 (every level keeps it), levels 1..5, npeaks 0..8.
 *
 *   mimc3_match_ncc_pyramid's definition word for word -- p_l = (u0 >> l, v0 >> l), d_{L-1} = floor((D + 2^{L-2}) / 2^{L-1}),
 *   d_{l-1} = 2 (d_l + s) with the level's arg-max cell s (a status -4 peak counts) or 2 d_l without one, shift_out = d_0 - offset, the
 *   +-2^24 bound on the starting displacement, the refusal of a coarsest level smaller than a chip (at the real ocw), the all-NaN record
 *   (and all-NaN candidate slots) for a level-0 box beyond the 256-px zero border, one stream and no host round trip.
 *   Levels.  Those of the pair's class -- the existing level sets, so levels built by mimc3_match_ncc_pyramid_dn / _pyramid_any serve
 *     this entry and the other way round:
 *       8-bit             the u8 levels with their u8 tables
 *       scaled-integer    the u16 levels with both tables
 *       integral f32      the integer-reduced f32 levels of mimc3_match_ncc_pyramid_dn
 *       any other pair    the float levels of mimc3_match_ncc_pyramid_any
 *   Kernel.  ONE kernel serves all levels of a call; mimc3_ctx_last_path reports it (mimc3_pyramid_chip_path gives the same value without
 *     a device: pair_class 0 8-bit, 1 scaled-integer, 2 integral f32, 3 any other; 0 for anything outside the table):
 *       pair class        mode 0                                                                         mode 1
 *       8-bit             at one of the six (7, 15, 16, 30, 32, 40): 6, exactly mimc3_match_ncc_pyramid_dn;   12 at every ocw
 *                         any other ocw: 12 (match_full_chip_u8_kernel.hip)
 *       scaled-integer    13 (match_full_chip_u16_kernel.hip) at every ocw, the six included             13 at every ocw
 *       integral f32      at the six: 8, mimc3_match_ncc_pyramid_dn; else 11 (match_full_chip_kernel.hip)    11 at every ocw
 *       any other         at the six: 9, mimc3_match_ncc_pyramid_any(mode 0); else 11                      11 at every ocw
 *     (The u16 matrix-core kernel never runs on an 8-bit pair here: the context keeps one integer level set per pair.  The mode-0 choice
 *      for a scaled-integer pair at the six is measured: on BASELINE C2 as 12-bit DN every pass of this entry was faster than every
 *      pass of mimc3_match_ncc_pyramid_dn at each of the six -- 25.9 against 104.4 ms at ocw 16, L = 3.)
 *     Levels L-1 .. 1 run that kernel's record-only form that also stores the arg-max cell (the matrix-core kernels as a clean launch
 *     over all points plus a masked launch over the points that hold a null: every point gets exactly one cell, or -1, per level);
 *     level 0 is the same kernel's record form, with candidates if asked, at shift = shift_out.
 *   Consequences.  On the three integer classes every sum is an exact integer in every kernel, so record, candidates and shift_out are
 *     the bytes of mimc3_match_ncc_pyramid_dn wherever that entry takes the call (the six), in both modes; at a chip size outside the six,
 *     record and candidates equal mimc3_match_ncc_full_chip_planes(mode 0, shift = shift_out) wherever that entry accepts the input.  On
 *     the float class, mode 0 at the six is mimc3_match_ncc_pyramid_any(mode 0); elsewhere shift_out equals a hand-made chain of
 *     mimc3_match_ncc_full_chip(mode 1, surf) calls over the float levels (arg-max of surf: the lowest k among the largest finite cells)
 *     and the record equals mimc3_match_ncc_full_chip(mode 1, shift = shift_out).
 *   Refusals: those of mimc3_match_ncc_pyramid_any, with ocw outside 1..mimc3_full_chip_max_ocw() in place of "not one of the six".
 *   Not covered: R > 15 on any level; several GPUs; MIMC3_hip_offsets (the command line keeps refusing levels > 1 at a chip size
 *   outside the six, 16-bit TIFFs, filter, peaks, fb and R > 15: the library entry is the way). */
int mimc3_match_ncc_pyramid_chip(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2],
                                 const int32_t *shift /*[N][2] or NULL*/, int32_t ocw, int32_t R, int32_t levels,
                                 int32_t npeaks /*0 = record only*/, int32_t swap, int32_t mode, float *out /*[N][8] host*/,
                                 float *cand /*[npeaks][N][3] host; NULL iff npeaks == 0*/, int32_t *shift_out /*[N][2] host or NULL*/);
/* Device-resident variant: the contract of mimc3_match_ncc_pyramid_any_dev. */
int mimc3_match_ncc_pyramid_chip_dev(mimc3_ctx *ctx, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                     const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap,
                                     int32_t mode, float *d_out, float *d_cand, int32_t *d_shift_out /*or NULL*/, void *stream);
/* Host query (no device): the mimc3_ctx_last_path value the table above gives, 0 for anything outside it. */
int mimc3_pyramid_chip_path(int32_t pair_class, int32_t ocw, int32_t mode);
/* FLOAT level `level` (1..4) of the pair the context currently matches on, whatever its class (mimc3_match_ncc_pyramid_any's levels), as
 * pixel values: out0, out1 [H >> level][W >> level] host.  Builds the float levels that are missing.  A level whose image would be
 * empty: MIMC3_EINVAL.  mimc3_ctx_get_pyramid_level keeps serving the integer levels, and keeps refusing a pair of no class. */
int mimc3_ctx_get_pyramid_level_any(mimc3_ctx *ctx, int32_t level, float *out0, float *out1);
/* Level `level` (1..4) of the pair the context currently matches on, as pixel values (w / 2^s): out0, out1 [H >> level][W >> level] host.
 * Builds the levels that are missing, for any of the three classes.  A pair of no class: MIMC3_EUNSUPPORTED; a level whose image would
 * be empty: MIMC3_EINVAL.  (For tests of the reduction.) */
int mimc3_ctx_get_pyramid_level(mimc3_ctx *ctx, int32_t level, float *out0, float *out1);
/* Host helper: the a-priori displacement as whole pixels, get_uv_pivot's sign convention (:559-598):
 *   shift[i] = (floor(vx dt / 365 / mpp + 0.5), floor(-vy dt / 365 / mpp + 0.5))   (f64, vx = xyuvav[i][4], vy = xyuvav[i][5]) */
int mimc3_prior_shift(const double *xyuvav, int32_t N, float dt, float mpp, int32_t *shift /*[N][2]*/);

/* ---- a2 on the device.  get_uv_pivot has two halves: the CORRIDOR of a point (theta = atan2(vy, vx), the normalised step,
 *      the corridor length, MIMC_module.c:559-573) needs libm and is computed on the host, bit-equal to the reference's;
 *      the pivot LIST (:576-598) is plain IEEE arithmetic on those numbers and is expanded by a kernel.  24 bytes per grid
 *      point cross PCIe instead of 8 bytes per pivot, and the lists never exist on the host.
 *      mimc3_pivot_corridors: cor = [N] records of MIMC3_CORRIDOR_BYTES bytes (host; opaque to the caller).
 *      mimc3_get_uv_pivot_dev: all pointers are device pointers; the context's image size bounds the pivots (as `i1` does in
 *      the reference).  Same two-call protocol as mimc3_get_uv_pivot (both list pointers NULL = offsets, total and extents
 *      only); d_piv_uv_neg (optional) receives the negated list main() makes in place for its swapped pass
 *      (MIMC_main.c:272-279).  extent[3] = what mimc3_pivot_extent returns.  Synchronises `stream` once (a 24-byte read-back).
 *      Results are bit-equal to mimc3_get_uv_pivot's. ----------------------------------------------------------------- */
#define MIMC3_CORRIDOR_BYTES 24
int mimc3_pivot_corridors(const double *xyuvav, int32_t N, float dt, float mpp, float aw_sf, float aw_cre, void *cor /*[N][24 B]*/);
int mimc3_get_uv_pivot_dev(mimc3_ctx *ctx, const double *d_xyuvav, const void *d_cor, int32_t N, int32_t ocw,
                           int64_t *d_piv_off /*[N+1]*/, int32_t *d_piv_uv /*[cap][2] or NULL*/, int32_t *d_piv_uv_neg /*[cap][2] or NULL*/,
                           int64_t cap, int64_t *total, int32_t extent[3], void *stream);
/* get_uv_pivot + matching_ncc_dlc_2 in one call, as main() pairs them (MIMC_main.c:264-267, :281-284): host buffers in and
 * out like mimc3_match_ncc_dlc, but the pivots are made on the device from the uploaded corridors.  `swap` != 0 is the
 * swapped pass: images exchanged AND the pivots negated (the caller still negates `offset` and the resulting (du, dv)). */
int mimc3_match_ncc_dlc_geo(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const int32_t offset[2], float dt, float mpp,
                            float aw_sf, float aw_cre, int32_t ocw, int32_t swap, float *out /*[N][3] host*/);
/* The same with the corridors made beforehand by mimc3_pivot_corridors (they do not depend on the chip size: main() would make
 * them once for its eight raw-image calls, as it makes the pivot lists once per chip size).  Per grid point 16 B of (u, v),
 * 24 B of corridor go up and 12 B of result come down; the grid is pipelined through in chunks, the transfers running under
 * the matcher.  Pinned `xyuvav`-independent: any host pointers work, pinned `cor` / `out` (mimc3_host_alloc) overlap best. */
int mimc3_match_ncc_dlc_cor(mimc3_ctx *ctx, const double *xyuvav, const void *cor /*[N][24 B] host*/, int32_t N, const int32_t offset[2],
                            int32_t ocw, int32_t swap, float *out /*[N][3] host*/);

/* ---- a8: neighbour offsets.  Replaces get_ruv_neighbor (MIMC_module.h:56, :1266-1327).
 *      Host code.  Returns the count in *nn; MIMC3_ECAP if it exceeds cap (pairs). ------------- */
int mimc3_get_ruv_neighbor(const double *xyuvav, int32_t N, int32_t dimx, int32_t dimy,
                           float meter_per_spacing, float radius, int32_t *ruv /*[cap][2]*/, int32_t cap,
                           int32_t *nn);

/* ---- a9-a10: QM pseudo-smoothing.  Replaces get_dpf_pseudosmoothing (MIMC_module.h:58,
 *      MIMC_module.c:1986-2312) incl. quadfit2 / GMA_double_inv.  In place on dpf, dpf_dx, dpf_dy
 *      ([dimy][dimx]).  mvn = candidates padded to [N][Kmax][5] (mean_u, mean_v, var_u, var_v,
 *      fraction) with nclus[N] valid rows (flattening of `GMA_float **mvn_dp`).
 *      max_sweeps: the reference loops while NOI<=100, i.e. at most 101 sweeps -> pass 101 for
 *      drop-in behaviour (BASELINE config C5 passes 10).  sweeps_done may be NULL. ------------- */
int mimc3_qm_pseudosmooth(mimc3_ctx *ctx, int32_t dimy, int32_t dimx, int32_t *dpf, float *dpf_dx, float *dpf_dy,
                          const int32_t *ruv, int32_t nn, const float *mvn, int32_t Kmax, const int32_t *nclus,
                          const double *xyuvav, int32_t max_sweeps, int32_t *sweeps_done);
/* Device-resident variant: d_work must hold mimc3_qm_workspace_bytes(dimy*dimx, max_sweeps) bytes.
 * Runs up to max_sweeps sweeps back-to-back with device-side early-out (no host sync). */
int64_t mimc3_qm_workspace_bytes(int32_t ngrid, int32_t max_sweeps);
int32_t mimc3_qm_launches_per_sweep(void);   /* kernel launches enqueued per sweep (2: fit + commit/compare/decide) */
int mimc3_qm_pseudosmooth_dev(mimc3_ctx *ctx, int32_t dimy, int32_t dimx, int32_t *d_dpf, float *d_dpf_dx,
                              float *d_dpf_dy, const int32_t *d_ruv, int32_t nn, const float *d_mvn, int32_t Kmax,
                              const int32_t *d_nclus, const double *d_xyuvav, int32_t max_sweeps,
                              void *d_work, int32_t *d_sweeps_done, void *stream);

/* ---- N1 (the stages between the 32 matcher passes and the QM update) ------------------------------
 *      Candidate clustering.  Replaces calc_mean_var_num_dp_cluster (MIMC_module.h:49, MIMC_module.c:994-1130)
 *      with cluster_euclidian / mark_row (:1133-1222).  dp = the ndp matcher outputs, pass-major
 *      [ndp][N][3] (flattening of `GMA_float **dp`), 1 <= ndp <= 64.  mvn out = [N][Kmax][5] (mean_u, mean_v,
 *      var_u, var_v, fraction; padding rows zero), nclus out = [N].  *kmax_seen = the largest cluster count;
 *      MIMC3_ECAP if it exceeds Kmax (Kmax = ndp is always enough). ------------------------------------ */
int mimc3_cluster_candidates(mimc3_ctx *ctx, const float *dp, int32_t ndp, int32_t N, int32_t Kmax, float *mvn,
                             int32_t *nclus, int32_t *kmax_seen);
int mimc3_cluster_candidates_dev(mimc3_ctx *ctx, const float *d_dp, int32_t ndp, int32_t N, int32_t Kmax,
                                 float *d_mvn, int32_t *d_nclus, int32_t *d_kmax_seen, void *stream);

/*      Prominent-cluster pick.  Replaces get_dpf0 (MIMC_module.h:52, MIMC_module.c:1224-1263):
 *      dpf[g] = first cluster whose fraction > min_ratio, else -1. ---------------------------------- */
int mimc3_get_dpf0(mimc3_ctx *ctx, const float *mvn, const int32_t *nclus, int32_t N, int32_t Kmax, float min_ratio,
                   int32_t *dpf);
int mimc3_get_dpf0_dev(mimc3_ctx *ctx, const float *d_mvn, const int32_t *d_nclus, int32_t N, int32_t Kmax,
                       float min_ratio, int32_t *d_dpf, void *stream);

/*      A-priori-guided fill of the unassigned points.  Replaces get_dpf1 (MIMC_module.h:54,
 *      MIMC_module.c:1330-1718).  dpf in = dpf0, out = dpf1 ([dimy][dimx]); dpf_dx, dpf_dy out.  dt, mpp = the
 *      reference's globals `dt` and `param_mimc2.mpp`.  The sweep count is data dependent and unbounded in
 *      the reference, so even the _dev variant synchronises `stream` once per 32 sweeps to poll the device's
 *      done flag; d_work must hold mimc3_dpf1_workspace_bytes(dimy*dimx).  sweeps_done (host, may be NULL)
 *      receives the reference's NOI. -------------------------------------------------------------------- */
int mimc3_get_dpf1(mimc3_ctx *ctx, int32_t dimy, int32_t dimx, int32_t *dpf, float *dpf_dx, float *dpf_dy,
                   const int32_t *ruv, int32_t nn, const float *mvn, int32_t Kmax, const int32_t *nclus,
                   const double *xyuvav, float dt, float mpp, int32_t *sweeps_done);
int64_t mimc3_dpf1_workspace_bytes(int32_t ngrid);
int mimc3_get_dpf1_dev(mimc3_ctx *ctx, int32_t dimy, int32_t dimx, int32_t *d_dpf, float *d_dpf_dx, float *d_dpf_dy,
                       const int32_t *d_ruv, int32_t nn, const float *d_mvn, int32_t Kmax, const int32_t *d_nclus,
                       const double *d_xyuvav, float dt, float mpp, void *d_work, int32_t *sweeps_done, void *stream);

/* ---- N2: image pre-filter.  Replaces GMA_float_conv2 (MIMC_module.h:67, MIMC_module.c:2517-2585): correlation
 *      with a kh x kw kernel (row-major, at most 81 taps) over the interior, a null DN poisoning its stencil,
 *      then `out -= min-1` / poisoned -> 0.  `out` [H][W] is IN/OUT exactly as in the reference: its border
 *      rows/columns are never written by the stencil but take part in the minimum and (right-hand columns) in
 *      the shift, so pass the buffer the reference would have (a fresh GMA_float_create plane: zeros).
 *      _dev: d_scratch = 4 bytes of device memory; enqueues on `stream`, no sync. ---------------------- */
int mimc3_float_conv2(mimc3_ctx *ctx, const float *in, int32_t H, int32_t W, const float *kernel, int32_t kh,
                      int32_t kw, float *out);
int mimc3_float_conv2_dev(mimc3_ctx *ctx, const float *d_in, int32_t H, int32_t W, const float *kernel /*host*/,
                          int32_t kh, int32_t kw, float *d_out, void *d_scratch, void *stream);
/*      Filter the context's resident pair on the device and make the filtered pair the one the matcher uses
 *      (what MIMC_main.c:302-350 does with host copies for its 24 filtered passes).  Like the reference, the two
 *      output planes are created once per pair (zeros) and REUSED by consecutive calls, so the border a filter
 *      leaves behind is input to the next one; mimc3_ctx_set_images* starts over, and so does kernel = NULL,
 *      which goes back to the pair as handed over (one run of the reference program = one such sequence).
 *      Nothing crosses PCIe.
 *      mimc3_ctx_get_images downloads the pair currently in use (either pointer may be NULL). --------- */
int mimc3_ctx_filter_images(mimc3_ctx *ctx, const float *kernel, int32_t kh, int32_t kw);
int mimc3_ctx_get_images(mimc3_ctx *ctx, float *i0, float *i1);

/* ---- N4: control-point offset.  Replaces get_offset_image (MIMC_module.h:34, MIMC_module.c:33-492) incl.
 *      GMA_double_randperm_row (:494-541).  Works on the context's resident pair AS HANDED OVER (any
 *      mimc3_ctx_filter_images state is ignored).  The reference's globals travel in mimc3_cp_params; its
 *      srand(time(NULL)) becomes `seed` (< 0 = time(NULL)), so a run can be repeated.  *status receives the
 *      reference's return value: 1 = offset valid, -1 = not enough control points (offset untouched; the CLI
 *      then gives up on the pair, MIMC_main.c:246-252).  flag_cp [N] bytes: set to 1 for every grid point that
 *      voted (never cleared: pass zeros, as GMA_uint8_create gives).  info (may be NULL) = #candidates, CP
 *      threshold, segments run, CPs found; sduv (may be NULL) = the two vote sums.
 *      MIMC3_EBOUNDS if a candidate's chip (+-(vec_ocw[2]+AW_CRE+3) px) leaves the image. ---------------- */
typedef struct mimc3_cp_params {
    int32_t vec_ocw[4];       /* param.vec_ocw: [1] and [2] are matched, [2] sizes the chips and the validity test */
    float aw_cre;             /* param.AW_CRE: rectangular pivot set -AW_CRE..AW_CRE in u and v                  */
    int32_t num_cp_max, num_cp_min;
    float ratio_cp, thres_spd_cp;
    const float *kernel[3];   /* the CLI's three pre-filter kernels (MIMC_main.c:176-194), row-major              */
    int32_t kdim[3][2];       /* rows, cols of each (at most 3 x 3)                                               */
    int64_t seed;
} mimc3_cp_params;
int mimc3_get_offset_image(mimc3_ctx *ctx, const double *xyuvav, int32_t N, const mimc3_cp_params *params,
                           int32_t offset[2], uint8_t *flag_cp, int32_t *status, int32_t *info /*[4]*/,
                           float *sduv /*[2]*/);
/*      The same stage with its device work shared by `nctx` contexts (one per GPU, each holding the SAME pair):
 *      the candidates of every segment are cut into nctx contiguous slices -- candidates are as independent as
 *      grid points (MIMC_module.c:325-378) -- which the contexts match side by side on host threads of their
 *      own.  What the reference does in sequence stays on the calling thread (the rand() shuffle, the segment
 *      loop and its early exit, the chip-to-chip recurrence of the filtered planes' minima, the f32 vote sums in
 *      candidate order): the result is that of the one-context call, whatever nctx is.  ctxs[0] does the
 *      candidate selection and the segment-wide minima.  mimc3_mgpu_vmap calls this with all of its ranks.    */
int mimc3_get_offset_image_multi(mimc3_ctx *const *ctxs, int32_t nctx, const double *xyuvav, int32_t N,
                                 const mimc3_cp_params *params, int32_t offset[2], uint8_t *flag_cp,
                                 int32_t *status, int32_t *info /*[4]*/, float *sduv /*[2]*/);

/* ---- N3: the program's data path on arrays ---------------------------------------------------------------
 *      mimc3_postprocess replaces mimc2_postprocess (MIMC_module.h:48, MIMC_module.c:892-990): clustering ->
 *      dpf0 (ratio 0.6) -> dpf1 (radius_dpf1) -> QM pseudo-smoothing (radius_ps, qm_max_sweeps: 101 = reference)
 *      -> out5 [5][dimy*dimx] = mean_u, mean_v, var_u, var_v, fraction of the chosen cluster, NaN where none
 *      (the reference's vxyexyqual[0..4] BEFORE main()'s unit conversion).  dp = [ndp][N][3] pass-major.
 *      _dev: d_dp, d_xyuvav, d_out5 on the device; xyuvav also on the host (neighbour geometry is host code);
 *      synchronises `stream` (data-dependent sweep counts, temporary buffers). ------------------------------ */
int mimc3_postprocess(mimc3_ctx *ctx, const float *dp, int32_t ndp, const double *xyuvav, int32_t dimx, int32_t dimy,
                      float dt, float mpp, float meter_per_spacing, float radius_dpf1, float radius_ps,
                      int32_t qm_max_sweeps, float *out5);
int mimc3_postprocess_dev(mimc3_ctx *ctx, const float *d_dp, int32_t ndp, const double *xyuvav, const double *d_xyuvav,
                          int32_t dimx, int32_t dimy, float dt, float mpp, float meter_per_spacing, float radius_dpf1,
                          float radius_ps, int32_t qm_max_sweeps, float *d_out5, void *stream);

/*      mimc3_vmap = MIMC_main.c:203-402, from "xyuvav and both images loaded" to "save the output", on the
 *      context's resident pair: grid geometry (:209-223), CP offset (:240-256), the 32 matcher passes
 *      (:261-350; pivots, images, candidates never leave the device), mimc2_postprocess (:353), removal of the
 *      sub-integer CP offset and px -> m/yr (:356-402).  Outputs [dimy*dimx] f32 as the reference saves them:
 *      vx, vy (m/yr, vy north-positive), ex, ey (m/yr), qual; flag_cp [N] bytes.  res->cp_status = -1 means
 *      "not enough control points": nothing else is computed (the CLI then touches vmap_*.tar, :248-252). --- */
typedef struct mimc3_vmap_params {
    int32_t vec_ocw[4];                 /* MIMC_main.c:134-137: 7, 15, 30, 40                        */
    float aw_cre, aw_sf;                /* :154-155: 10.0, 1.8                                        */
    float radius_neighbor_dpf1;         /* :164: 1000/300 = 3 (grid spacings)                         */
    float radius_neighbor_ps;           /* :165: 5.0                                                  */
    int32_t num_cp_max, num_cp_min;     /* :168-169: 500, 50                                          */
    float ratio_cp, thres_spd_cp;       /* :170-171: 0.03, 10                                         */
    const float *kernel[3];             /* :176-194: d/dx 1x3, d/dy 3x1, Laplacian 3x3, row-major     */
    int32_t kdim[3][2];
    int64_t cp_seed;                    /* shuffle seed of the CP stage; < 0 = time(NULL)             */
    int32_t qm_max_sweeps;              /* 0 or 101 = reference                                        */
} mimc3_vmap_params;
typedef struct mimc3_vmap_result {
    int32_t dimx, dimy;
    float mpp, spacing_grid, meter_per_spacing;
    int32_t cp_status;                  /* 1 ok, -1 not enough control points                         */
    int32_t offset_cp[2];               /* integer CP offset (meta: cp_offset_int_u/v)                */
    float cp_subint[2];                 /* grid mean removed afterwards (meta: cp_offset_subint_u/v)  */
} mimc3_vmap_result;
int mimc3_vmap(mimc3_ctx *ctx, const double *xyuvav, int32_t N, float dt, const mimc3_vmap_params *params,
               float *vx, float *vy, float *ex, float *ey, float *qual, uint8_t *flag_cp, mimc3_vmap_result *res);
/*      The same in two steps, for a multi-GPU driver (grid points are independent in the matcher):
 *      mimc3_vmap_passes = geometry + CP offset on the WHOLE grid + the 32 passes for grid points [lo, hi) only, into
 *      d_dp [32][hi-lo][3] (device, pass-major); the caller all-gathers the blocks into [32][N][3] and every rank
 *      calls mimc3_vmap_finish (post-processing, unit conversion) with the `res` its own passes call filled.
 *      mimc3_vmap is passes(0, N) + finish. ---------------------------------------------------------------------- */
int mimc3_vmap_passes(mimc3_ctx *ctx, const double *xyuvav, int32_t N, float dt, const mimc3_vmap_params *params,
                      int32_t lo, int32_t hi, float *d_dp, uint8_t *flag_cp, mimc3_vmap_result *res);
int mimc3_vmap_finish(mimc3_ctx *ctx, const double *xyuvav, int32_t N, float dt, const mimc3_vmap_params *params,
                      const float *d_dp, float *vx, float *vy, float *ex, float *ey, float *qual, mimc3_vmap_result *res);
/*      ... and in finer pieces, for a driver that measures the CP offset ONCE and shards by cost-balanced point sets:
 *      mimc3_vmap_geometry = grid geometry only (:209-223); mimc3_vmap_cp = geometry + CP offset (:240-256) -> res, flag_cp;
 *      mimc3_vmap_passes_points = host pivots + the 32 passes for ANY set of grid points xs [n][6] with the CP offset in
 *      `res`, into d_dp [32][pass_stride][3] (pass_stride >= n points per pass slot; 0 = n). -------------------------------- */
int mimc3_vmap_geometry(const double *xyuvav, int32_t N, mimc3_vmap_result *res);
int mimc3_vmap_cp(mimc3_ctx *ctx, const double *xyuvav, int32_t N, float dt, const mimc3_vmap_params *params, uint8_t *flag_cp,
                  mimc3_vmap_result *res);
int mimc3_vmap_passes_points(mimc3_ctx *ctx, const double *xs, int32_t n, float dt, const mimc3_vmap_params *params,
                             const mimc3_vmap_result *res, float *d_dp, int64_t pass_stride);

/* ---- e: multi-GPU.  The loop that shards is the reference's OpenMP loop over grid points (MIMC_module.c:816-838): grid
 *      points are independent in the matcher, so each GPU matches its own share against the replicated pair and ONE
 *      all-gather re-assembles the result.  Two forms:
 *      (1) one process per GPU (torch.distributed / MPI launchers): mimc3_vmap_passes + the caller's own all-gather +
 *          mimc3_vmap_finish, above;
 *      (2) ONE process driving several GPUs, here: a host thread per device and an RCCL communicator over them
 *          (ncclCommInitAll; RCCL -- librccl.so.1 -- is loaded with dlopen on first use).
 *          The MIMC3_hip command line takes this form with MIMC3_HIP_DEVICES=0,1,...
 *      Shares are cost-balanced: mimc3_point_cost adds (4 + 6 npiv)(2 ocw + 1)^2 per point (NCC evaluations x chip area),
 *      mimc3_partition_points cuts the grid into blocks of `block` consecutive points, deals them heaviest-first to the
 *      least loaded rank and returns order[start[r] .. start[r+1]) = the points of rank r (each rank's blocks in grid
 *      order); *imbalance = max load / mean load - 1.  Host code. ------------------------------------------------------ */
int mimc3_point_cost(const int64_t *piv_off, int32_t N, int32_t ocw, double *cost /*[N], accumulated*/);
int mimc3_partition_points(const double *cost, int32_t N, int32_t world, int32_t block, int32_t *order /*[N]*/,
                           int32_t *start /*[world+1]*/, double *imbalance /*may be NULL*/);
typedef struct mimc3_mgpu mimc3_mgpu;
int  mimc3_mgpu_create(const int32_t *devices, int32_t ndev, mimc3_mgpu **out);   /* a context per device + the communicator */
/* Test / bring-up form of the above (the product entry point never takes these, and the library reads neither from the environment):
 * comm_lib = a library exporting the six RCCL entry points the driver uses (NULL: RCCL); MIMC3_MGPU_REPEAT_DEVICES in flags lets a
 * device be listed more than once (N ranks as N contexts of one GPU over a stand-in communicator). */
#define MIMC3_MGPU_REPEAT_DEVICES 1u
int  mimc3_mgpu_create_ex(const int32_t *devices, int32_t ndev, const char *comm_lib, uint32_t flags, mimc3_mgpu **out);
void mimc3_mgpu_destroy(mimc3_mgpu *mg);
int32_t mimc3_mgpu_ndev(mimc3_mgpu *mg);
mimc3_ctx *mimc3_mgpu_ctx(mimc3_mgpu *mg, int32_t rank);
double mimc3_mgpu_last_imbalance(mimc3_mgpu *mg);                                 /* of the last call's partition */
/*      the pair, replicated on every device (uploads run in parallel) */
int mimc3_mgpu_set_images(mimc3_mgpu *mg, const float *i0, const float *i1, int32_t H, int32_t W);
int mimc3_mgpu_set_images_u8(mimc3_mgpu *mg, const uint8_t *i0, const uint8_t *i1, int32_t H, int32_t W);
int mimc3_mgpu_set_images_u16(mimc3_mgpu *mg, const uint16_t *i0, const uint16_t *i1, int32_t H, int32_t W);
/*      mimc3_match_ncc_dlc / mimc3_vmap with the grid points sharded over the devices; same arguments, same results
 *      (bit-identical: a point's result does not depend on which device computes it).  The CP offset of mimc3_mgpu_vmap
 *      is measured once, on device 0; post-processing runs on device 0. */
int mimc3_mgpu_match_ncc_dlc(mimc3_mgpu *mg, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *piv_uv,
                             const int64_t *piv_off, int32_t ocw, int32_t swap, float *out /*[N][3] host*/);
int mimc3_mgpu_vmap(mimc3_mgpu *mg, const double *xyuvav, int32_t N, float dt, const mimc3_vmap_params *params, float *vx, float *vy,
                    float *ex, float *ey, float *qual, uint8_t *flag_cp, mimc3_vmap_result *res);

/*      small device helpers the driver is built from: the context's own stream; (du,dv) -> (-du,-dv) of a swapped
 *      pass (MIMC_main.c:289-293); cluster map -> five planes (mimc2_postprocess :937-970 /
 *      convert_dpf_to_vxy_exy_qual, MIMC_module.h:64); size of the resident pair. --------------------------- */
void *mimc3_ctx_stream(mimc3_ctx *ctx);
int mimc3_negate_uv_dev(mimc3_ctx *ctx, float *d_out, int32_t N, void *stream);
int mimc3_negate_pivots_dev(mimc3_ctx *ctx, const int32_t *d_piv_uv, int32_t *d_out /*[count][2]*/, int64_t count, void *stream); /* :272-279 */
int mimc3_dpf_to_vxyexyqual_dev(mimc3_ctx *ctx, const int32_t *d_dpf, const float *d_mvn, int32_t N, int32_t Kmax,
                                float *d_out5, void *stream);
int mimc3_ctx_image_size(mimc3_ctx *ctx, int32_t *H, int32_t *W);
int mimc3_ctx_device(mimc3_ctx *ctx);
/*      device scratch owned by the context: slot 0..15, grows on demand, contents kept until the slot is asked for more
 *      bytes; freed with the context.  The drivers above the ABI (mimc3_postprocess, mimc3_vmap) keep their working
 *      buffers here instead of allocating per call.  One stream at a time per context. */
int mimc3_ctx_workspace(mimc3_ctx *ctx, int32_t slot, size_t bytes, void **d_ptr);
/*      one of the context's four auxiliary hipStream_t (k = 0..3; created with the context -- creating a stream while
 *      kernels run costs milliseconds): the drivers' host threads upload on them next to the context's own stream. */
void *mimc3_ctx_aux_stream(mimc3_ctx *ctx, int32_t k);
/*      the same for PINNED host memory (slot 0..7): pinning pages costs milliseconds per tens of MB, so the drivers keep
 *      their staging buffers (the pivot lists of the 32 passes) across calls.  Distinct slots may be asked for from
 *      distinct host threads at the same time. */
int mimc3_ctx_host_workspace(mimc3_ctx *ctx, int32_t slot, size_t bytes, void **h_ptr);

/* ---- measurement helper: average device time (ms) of the last matcher launch sequence,
 *      taken with hipEvents on the launch stream (bench.py's roofline leg). -------------------- */
int mimc3_ctx_enable_timing(mimc3_ctx *ctx, int32_t on);
int mimc3_ctx_last_kernel_ms(mimc3_ctx *ctx, float *ms);

const char *mimc3_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MIMC3_HIP_H */
