// MIMC3_hip_offsets -- exhaustive-search NCC offsets with peak quality over libmimc3_hip.so (MI355X): the AMPCOR-style table that
// MIMC_single_match.c:1-27 describes.
//
//     MIMC3_hip_offsets <i0.tif> <i1.tif> <xyuvav.GMA> <outdir> [ocw=15] [R=15] [levels=1] [peaks=1] [filter=0] [fb=0]
//
// Inputs as for MIMC3_hip (the file names start with YYYYMMDDhhmmss; dt from the two timestamps); both images 8-bit, or both 16-bit
// (see below).  Steps: the
// control-point offset (mimc3_vmap_cp, as the reference program measures it), the a-priori shift of every grid point
// (mimc3_prior_shift), then every offset in [-R, R]^2 around uv0 + offset + shift (mimc3_match_ncc_full; R > 15: see below), or -- levels > 1 -- the
// coarse-to-fine search that starts there on a pair reduced levels - 1 times (mimc3_match_ncc_pyramid: a reach of about
// R (2^levels - 1) px).  Outputs in <outdir>:
//   offsets_<t0>_<t1>.GMA  f32 [N][10]: the [N][8] record of mimc3_match_ncc_full / _pyramid (du, dv, ncc_peak / status, ncc_fit, snr,
//                          h_uu, h_uv, h_vv) and u, v of the grid point
//   offsets_<t0>_<t1>.txt  the points with a non-negative status, one per line, AMPCOR's column order: u du v dv snr h_uu h_vv h_uv;
//                          du, dv there are the whole displacement (the control-point offset added); a first comment line names
//                          the columns and the offset
//   candidates_<t0>_<t1>.GMA  peaks = K > 1 (with levels = 1 only): f32 [K N][3], pass-major -- row j N + i = candidate j of grid point i,
//                          (du, dv, ncc) of its j-th best correlation peak (mimc3_match_ncc_full_multi): the dp of the post-matcher chain.
//                          peaks = 1 writes exactly the two files above
// filter = k in 1..3 (with levels = 1 only): the control-point offset is measured as before, then the pair is filtered on the device with
//   the reference program's k-th kernel (MIMC_main.c:176-194: d/dx, d/dy, Laplacian) and searched on the filtered pair
//   (mimc3_match_ncc_full_planes); the files are offsets_<t0>_<t1>_f<k>.GMA / .txt and candidates_<t0>_<t1>_f<k>.GMA.  filter = 0 writes
//   exactly the files of a run without the argument
// Two 16-bit TIFFs (levels = 1 only: the pyramid stays 8-bit): the same steps and the same files, the search through
//   mimc3_match_ncc_full_dn, which takes whatever the files hold -- 16-bit DN, or 8- and 12-bit DN in a 16-bit container -- raw or
//   filtered.  One 8-bit and one 16-bit file are refused
// fb = 1 (with levels = 1 only): the forward-backward consistency of every result (mimc3_match_ncc_full_fb: the same search, then every
//   record and candidate matched back from where it landed) is also written, as fb_<t0>_<t1>.GMA (fb_<t0>_<t1>_f<k>.GMA with a filter): f32
//   [(1 + K) N][4], plane-major, K = 0 for peaks = 1 and peaks otherwise -- row p N + i = (du_b, dv_b, ncc_b or status, err) of grid
//   point i's record (p = 0) or candidate p - 1.  fb = 0 writes exactly the files of a run without the argument
// R = 16 .. mimc3_wide_max_radius(ocw) (47; 39 at ocw 40; with levels = 1 only): one exact pass over the whole range
//   (mimc3_match_ncc_wide_planes in mode 0: a raw 8-bit pair, a filtered pair and a 12-bit pair in a 16-bit TIFF on the matrix cores, every
//   other pair on the float wide kernel -- the bytes of mimc3_match_ncc_wide either way; with fb = 1 mimc3_match_ncc_wide_fb) on 8-bit and 16-bit pairs, raw or filtered; the same files, peaks and
//   filter as above.  R <= 15 takes exactly the calls of a build without this range and writes the same bytes
// ocw = 1 .. mimc3_full_chip_max_ocw() (80) other than 7, 15, 16, 30, 32, 40 (with levels = 1, fb = 0 and R <= 15 only): the search through
//   mimc3_match_ncc_full_chip_planes (mode 0: an 8-bit or scaled-integer pair on the matrix cores, every other on the float kernel; the bytes of
//   mimc3_match_ncc_full_chip) on 8-bit and 16-bit pairs, raw or filtered; the same files, peaks and filter as above.  One of the
//   six takes exactly the calls of a build without this range and writes the same bytes
// Environment: MIMC3_HIP_DEVICE (default 0), MIMC3_CP_SEED (as for MIMC3_hip).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <unistd.h>
#include "../../../include/mimc3_hip.h"

#include "cli_io.h"

int main(int argc, char *argv[])
{
    printf("MIMC3_hip_offsets -- MI355X build (%s)\n", mimc3_version());
    if (argc < 5 || argc > 11) {
        fprintf(stderr, "usage: %s <i0.tif> <i1.tif> <xyuvav.GMA> <outdir> [ocw=15] [R=15] [levels=1] [peaks=1] [filter=0] [fb=0]\n", argv[0]);
        return 2;
    }
    const int32_t ocw = argc > 5 ? atoi(argv[5]) : 15, R = argc > 6 ? atoi(argv[6]) : 15, levels = argc > 7 ? atoi(argv[7]) : 1;
    const int32_t peaks = argc > 8 ? atoi(argv[8]) : 1;
    const int32_t filter = argc > 9 ? atoi(argv[9]) : 0;
    if (filter < 0 || filter > 3) { fprintf(stderr, "filter must be 0 (raw), 1 (d/dx), 2 (d/dy) or 3 (Laplacian)\n"); return 2; }
    if (filter != 0 && levels != 1) {
        fprintf(stderr, "filter > 0 needs levels = 1: the coarse-to-fine search runs on the raw 8-bit pair only\n");
        return 2;
    }
    const int32_t fbk = argc > 10 ? atoi(argv[10]) : 0;
    if (fbk != 0 && fbk != 1) { fprintf(stderr, "fb must be 0 or 1\n"); return 2; }
    if (fbk != 0 && levels != 1) {
        fprintf(stderr, "fb = 1 needs levels = 1: the forward-backward check runs on the single-level search only\n");
        return 2;
    }
    if (peaks != 1 && levels != 1) {
        fprintf(stderr, "peaks > 1 needs levels = 1: candidates on a pyramid's level 0 are not supported\n");
        return 2;
    }
    const bool any_chip = mimc3_wide_max_radius(ocw) == 0;     // not one of the six built chip sizes: the run-time-ocw entry
    if (any_chip) {
        const int32_t max_ocw = mimc3_full_chip_max_ocw();
        if (ocw < 1 || ocw > max_ocw) { fprintf(stderr, "ocw must be in 1..%d (mimc3_full_chip_max_ocw)\n", max_ocw); return 2; }
        if (levels != 1) {
            fprintf(stderr, "ocw %d needs levels = 1: the coarse-to-fine search takes ocw 7, 15, 16, 30, 32 or 40 only\n", ocw);
            return 2;
        }
        if (fbk != 0) {
            fprintf(stderr, "ocw %d needs fb = 0: the forward-backward check takes ocw 7, 15, 16, 30, 32 or 40 only\n", ocw);
            return 2;
        }
        if (R > 15) {
            fprintf(stderr, "ocw %d needs R <= 15: the search beyond +-15 px takes ocw 7, 15, 16, 30, 32 or 40 only\n", ocw);
            return 2;
        }
    }
    const bool wide = R > 15;               // beyond +-15 px: the wide entries, whatever the pixel class
    if (wide) {
        const int32_t max_r = mimc3_wide_max_radius(ocw);
        if (max_r == 0) { fprintf(stderr, "R > 15 needs ocw one of 7, 15, 16, 30, 32, 40\n"); return 2; }
        if (R > max_r) { fprintf(stderr, "R must be at most %d at ocw %d (mimc3_wide_max_radius)\n", max_r, ocw); return 2; }
        if (levels != 1) {
            fprintf(stderr, "R > 15 needs levels = 1: the coarse-to-fine search keeps R <= 15 on every level\n");
            return 2;
        }
    }
    char t0[15], t1[15];
    if (!timestamp_of(argv[1], t0) || !timestamp_of(argv[2], t1)) {
        fprintf(stderr, "image paths must contain a '/' and the file names must start with YYYYMMDDhhmmss\n");
        return 2;
    }
    const float dt = (float)(datenum(t1) - datenum(t0));
    const std::string tag = std::string(t0) + "_" + t1 + (filter ? "_f" + std::to_string(filter) : std::string());
    const std::string base = std::string(argv[4]) + "/offsets_" + tag;
    std::vector<double> xy;
    int32_t N = 0, ncol = 0;
    if (!load_gma_double(argv[3], xy, N, ncol) || ncol != 6) { fprintf(stderr, "cannot read %s as an [N][6] float64 .GMA\n", argv[3]); return 2; }
    RawImage i0, i1;
    if (!load_tiff(argv[1], i0) || !load_tiff(argv[2], i1)) { fprintf(stderr, "cannot read the TIFF images\n"); return 2; }
    if (i0.H != i1.H || i0.W != i1.W) { fprintf(stderr, "the two images differ in size\n"); return 2; }
    if (i0.bpp != i1.bpp || (i0.bpp != 1 && i0.bpp != 2)) {
        fprintf(stderr, "the exhaustive search takes two 8-bit or two 16-bit images\n");
        return 2;
    }
    const bool dn16 = i0.bpp == 2;
    if (dn16 && levels != 1) {
        fprintf(stderr, "16-bit images need levels = 1: the coarse-to-fine search runs on 8-bit pairs only\n");
        return 2;
    }
    const char *dev = getenv("MIMC3_HIP_DEVICE");
    mimc3_ctx *ctx = nullptr;
    auto leave = [&](int code) -> int {        // (as MIMC3_hip: no runtime teardown on the way out)
        fflush(nullptr);
        _exit(code);
    };
    if (mimc3_ctx_create(dev ? atoi(dev) : 0, &ctx) ||
        (dn16 ? mimc3_ctx_set_images_u16(ctx, reinterpret_cast<const uint16_t *>(i0.px.data()), reinterpret_cast<const uint16_t *>(i1.px.data()), i0.H, i0.W)
              : mimc3_ctx_set_images_u8(ctx, i0.px.data(), i1.px.data(), i0.H, i0.W))) {
        fprintf(stderr, "%s\n", mimc3_last_error());
        return leave(3);
    }
    // the control-point offset, as the reference program measures it (MIMC_main.c:240-256)
    const mimc3_vmap_params p = reference_vmap_params();
    std::vector<uint8_t> flag(N);
    mimc3_vmap_result r{};
    if (mimc3_vmap_cp(ctx, xy.data(), N, dt, &p, flag.data(), &r)) { fprintf(stderr, "%s\n", mimc3_last_error()); return leave(3); }
    int32_t offset[2] = {0, 0};
    if (r.cp_status < 0) printf("Not enough control points: searching around the a-priori displacement alone\n");
    else { offset[0] = r.offset_cp[0]; offset[1] = r.offset_cp[1]; }
    printf("dt=%f days, MPP=%f; control-point offset [%d, %d] pixels (i1-i0); ocw=%d, R=%d, %d grid points\n", dt, r.mpp, offset[0],
           offset[1], ocw, R, N);
    if (levels != 1) printf("coarse-to-fine over %d pyramid levels\n", levels);
    if (filter) {                              // the reference program's filter kernels (MIMC_main.c:176-194), in its order
        static const float gx[3] = {-1, 0, 1}, lap[9] = {-0.125f, -0.125f, -0.125f, -0.125f, 1, -0.125f, -0.125f, -0.125f, -0.125f};
        const int rcf = filter == 1 ? mimc3_ctx_filter_images(ctx, gx, 1, 3) : filter == 2 ? mimc3_ctx_filter_images(ctx, gx, 3, 1)
                                                                                             : mimc3_ctx_filter_images(ctx, lap, 3, 3);
        if (rcf) { fprintf(stderr, "%s\n", mimc3_last_error()); return leave(3); }
        printf("searching on the pair filtered with kernel %d\n", filter);
    }
    std::vector<int32_t> shift(2 * (size_t)N);
    std::vector<float> rec(8 * (size_t)N);
    std::vector<float> cand(peaks != 1 ? 3 * (size_t)(peaks > 0 ? peaks : 0) * (size_t)N : 0);
    if (peaks != 1) printf("the %d best correlation peaks of every grid point as candidates\n", peaks);
    const int32_t K = peaks != 1 ? (peaks > 0 ? peaks : 0) : 0;
    std::vector<float> fb(fbk ? 4 * (size_t)(1 + K) * (size_t)N : 0);
    if (fbk) printf("forward-backward consistency of every result\n");
    if (wide) printf("one exact pass over +-%d px\n", R);
    if (any_chip) printf("chip half-width %d: the run-time-ocw search kernel\n", ocw);
    if (mimc3_prior_shift(xy.data(), N, dt, r.mpp, shift.data()) ||
        (wide ? (fbk ? mimc3_match_ncc_wide_fb(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks != 1 ? peaks : 0, rec.data(),
                                               K > 0 ? cand.data() : nullptr, fb.data())
                     : mimc3_match_ncc_wide_planes(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks != 1 ? peaks : 0, 0, 0, rec.data(),
                                                   K > 0 ? cand.data() : nullptr, nullptr))
         : any_chip ? mimc3_match_ncc_full_chip_planes(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks != 1 ? peaks : 0, 0, 0, rec.data(),
                                                       K > 0 ? cand.data() : nullptr, nullptr)
         : fbk ? mimc3_match_ncc_full_fb(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks != 1 ? peaks : 0, 0, rec.data(),
                                       K > 0 ? cand.data() : nullptr, fb.data())
         : dn16 ? mimc3_match_ncc_full_dn(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks != 1 ? peaks : 0, 0, rec.data(),
                                        peaks != 1 ? cand.data() : nullptr)
         : filter ? mimc3_match_ncc_full_planes(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks != 1 ? peaks : 0, 0, rec.data(),
                                                peaks != 1 ? cand.data() : nullptr)
         : peaks != 1 ? mimc3_match_ncc_full_multi(ctx, xy.data(), N, offset, shift.data(), ocw, R, peaks, 0, rec.data(), cand.data())
         : levels == 1 ? mimc3_match_ncc_full(ctx, xy.data(), N, offset, shift.data(), ocw, R, 0, rec.data())
                       : mimc3_match_ncc_pyramid(ctx, xy.data(), N, offset, shift.data(), ocw, R, levels, 0, rec.data(), nullptr))) {
        fprintf(stderr, "%s\n", mimc3_last_error());
        return leave(3);
    }
    std::vector<float> out(10 * (size_t)N);
    int32_t nok = 0;
    for (int32_t g = 0; g < N; g++) {
        for (int k = 0; k < 8; k++) out[10 * (size_t)g + k] = rec[8 * (size_t)g + k];
        out[10 * (size_t)g + 8] = (float)xy[6 * (size_t)g + 2];
        out[10 * (size_t)g + 9] = (float)xy[6 * (size_t)g + 3];
        nok += rec[8 * (size_t)g + 2] >= -1.0f;
    }
    bool ok = save_gma(base + ".GMA", out.data(), N, 10);
    if (peaks != 1) ok = save_gma(std::string(argv[4]) + "/candidates_" + tag + ".GMA", cand.data(), peaks * N, 3) && ok;
    if (fbk) ok = save_gma(std::string(argv[4]) + "/fb_" + tag + ".GMA", fb.data(), (1 + K) * N, 4) && ok;
    FILE *f = fopen((base + ".txt").c_str(), "w");
    if (f) {
        fprintf(f, "# u du v dv snr h_uu h_vv h_uv   (du, dv include the control-point offset %d %d)\n", offset[0], offset[1]);
        for (int32_t g = 0; g < N; g++) {
            const float *q = rec.data() + 8 * (size_t)g;
            if (!(q[2] >= -1.0f)) continue;
            fprintf(f, "%d %.4f %d %.4f %.5f %.6g %.6g %.6g\n", (int)xy[6 * (size_t)g + 2], q[0] + (float)offset[0], (int)xy[6 * (size_t)g + 3],
                    q[1] + (float)offset[1], q[4], q[5], q[7], q[6]);
        }
        ok = fclose(f) == 0 && ok;
    } else ok = false;
    if (!ok) { fprintf(stderr, "could not write the outputs under %s\n", argv[4]); return leave(4); }
    printf("%d of %d grid points with a peak; written %s.GMA and %s.txt\n", nok, N, base.c_str(), base.c_str());
    return leave(0);
}
