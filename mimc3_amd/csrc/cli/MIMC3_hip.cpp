// MIMC3_hip -- the reference program's command line over libmimc3_hip.so (MI355X).
//
//     MIMC3_hip <i0.tif> <i1.tif> <xyuvav.GMA> <outdir>
//
// Same arguments, same files in <outdir>, same exit behaviour as the reference's main() (MIMC_main.c:43-528):
//   * image paths must contain a '/' and their basename must start with YYYYMMDDhhmmss (getTimeStampStr,
//     MIMC_misc.c:133-153); dt = difference of the two timestamps in days (get_datenum / get_dt, :27-131)
//   * <outdir>/vmap_<t0>_<t1>.tar already there -> "vmap already exists. Skipping", exit -1 (:122-130)
//   * not enough control points -> an empty vmap_<t0>_<t1>.tar is created, exit -1 (:246-252)
//   * outputs: vmap_<t0>_<t1>_{x,y}.GMA (f64 1 x dim), _{vx,vy,ex,ey,qual}.GMA (f32 dimy x dimx), _flagcp.GMA (u8),
//     _meta.txt (7 key=value lines) (:404-447)
// Everything between "inputs loaded" and "save the output" is mimc3_vmap() on the GPU; there is no CPU path.
// Environment: MIMC3_HIP_DEVICE (default 0); MIMC3_HIP_DEVICES=0,1,... shards the grid points over several GPUs of the node
// (one host thread per device, RCCL all-gather of the candidate blocks: mimc3_mgpu_vmap); MIMC3_CP_SEED (pin the
// control-point shuffle; default time(NULL) like the reference).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <chrono>
#include <thread>
#include <unistd.h>
#include <tiffio.h>
#include "../../../include/mimc3_hip.h"

#include "cli_io.h"

int main(int argc, char *argv[])
{
    const char ver[] = "3.0.7";        // the reference version whose outputs this build reproduces (meta key MIMC_version)
    printf("\n\nMIMC version %s -- MI355X build (%s)\n\n", ver, mimc3_version());
    if (argc != 5) {
        fprintf(stderr, "usage: %s <i0.tif> <i1.tif> <xyuvav.GMA> <outdir>\n", argv[0]);
        return 2;
    }
    char t0[15], t1[15];
    if (!timestamp_of(argv[1], t0) || !timestamp_of(argv[2], t1)) {
        fprintf(stderr, "image paths must contain a '/' and the file names must start with YYYYMMDDhhmmss\n");
        return 2;
    }
    const std::string base = std::string(argv[4]) + "/vmap_" + t0 + "_" + t1;
    const std::string f_tar = base + ".tar";
    const float dt = (float)(datenum(t1) - datenum(t0));                                // get_dt, MIMC_misc.c:121-131
    printf("dt=%f days\n\nEarlier image: %s\nLatter image: %s\nxyuvav matrix: %s\n", dt, argv[1], argv[2], argv[3]);
    if (access(f_tar.c_str(), F_OK) == 0) {                                             // :122-130
        printf("vmap already exists. Skipping\n");
        return -1;
    }

    // ---- parameters and kernels (:134-194)
    const mimc3_vmap_params p = reference_vmap_params();

    // MIMC3_CLI_TIMING=1: wall time of each step on stderr
    const bool timing = getenv("MIMC3_CLI_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[MIMC3_hip] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    // ---- inputs (:200-230)
    std::vector<double> xy;
    int32_t N = 0, ncol = 0;
    if (!load_gma_double(argv[3], xy, N, ncol) || ncol != 6) { fprintf(stderr, "cannot read %s as an [N][6] float64 .GMA\n", argv[3]); return 2; }
    // the HIP runtime and the device context(s) come up on a second thread while this one decodes the TIFFs
    const char *dev = getenv("MIMC3_HIP_DEVICE");
    std::vector<int32_t> devs;
    if (const char *dl = getenv("MIMC3_HIP_DEVICES")) {
        for (const char *q = dl; *q;) {
            char *end = nullptr;
            const long v = strtol(q, &end, 10);
            if (end == q) break;
            devs.push_back((int32_t)v);
            q = (*end == ',') ? end + 1 : end;
        }
        if (devs.empty()) { fprintf(stderr, "MIMC3_HIP_DEVICES: expected a comma-separated list of device ordinals\n"); return 2; }
    }
    mimc3_ctx *ctx = nullptr;
    mimc3_mgpu *mg = nullptr;
    int ctx_rc = 0;
    std::string ctx_err;
    std::thread ctx_thread([&]() {
#ifdef MIMC3_TEST_HOOKS      // test build only (tests/_build/MIMC3_hip_test): N ranks on one device over a stand-in communicator
        if (!devs.empty() && (getenv("MIMC3_TEST_COMM_LIB") || getenv("MIMC3_TEST_REPEAT"))) {
            const char *rp = getenv("MIMC3_TEST_REPEAT");
            ctx_rc = mimc3_mgpu_create_ex(devs.data(), (int32_t)devs.size(), getenv("MIMC3_TEST_COMM_LIB"), (rp && rp[0] == '1') ? MIMC3_MGPU_REPEAT_DEVICES : 0u, &mg);
        } else
#endif
        ctx_rc = devs.empty() ? mimc3_ctx_create(dev ? atoi(dev) : 0, &ctx) : mimc3_mgpu_create(devs.data(), (int32_t)devs.size(), &mg);
        if (ctx_rc) ctx_err = mimc3_last_error();
    });
    auto cleanup = [&]() { if (ctx) mimc3_ctx_destroy(ctx); if (mg) mimc3_mgpu_destroy(mg); ctx = nullptr; mg = nullptr; };
    // Every exit once the device context may exist goes through here: flush, then _exit.  Returning from main() would run
    // the static destructors of the HIP runtime (and of RCCL with MIMC3_HIP_DEVICES) with contexts, streams and communicators
    // still alive -- on some RCCL versions that hangs or aborts, turning a clean error code into a signal.
    auto leave = [&](int code) -> int {
        fflush(nullptr);
        if (getenv("MIMC3_CLI_TEARDOWN")) { cleanup(); return code; }     // (leak checkers)
        _exit(code);
    };
    RawImage i0, i1;
    lap("xyuvav read");
    const bool tiff_ok = load_tiff(argv[1], i0) && load_tiff(argv[2], i1);
    lap("TIFF decode");
    ctx_thread.join();
    lap("device context (rest of)");
    if (!tiff_ok) { fprintf(stderr, "cannot read the TIFF images\n"); return leave(2); }
    if (i0.H != i1.H || i0.W != i1.W) { fprintf(stderr, "the two images differ in size\n"); return leave(2); }
    if (ctx_rc) { fprintf(stderr, "%s\n", ctx_err.c_str()); return leave(3); }
    const int32_t H = i0.H, W = i0.W;
    int rc;
    if (i0.bpp == 1 && i1.bpp == 1)
        rc = mg ? mimc3_mgpu_set_images_u8(mg, i0.px.data(), i1.px.data(), H, W) : mimc3_ctx_set_images_u8(ctx, i0.px.data(), i1.px.data(), H, W);
    else if (i0.bpp == 2 && i1.bpp == 2) {
        const uint16_t *q0 = reinterpret_cast<const uint16_t *>(i0.px.data()), *q1 = reinterpret_cast<const uint16_t *>(i1.px.data());
        rc = mg ? mimc3_mgpu_set_images_u16(mg, q0, q1, H, W) : mimc3_ctx_set_images_u16(ctx, q0, q1, H, W);
    } else {                                  // one 8-bit and one 16-bit file: widen on the host like the reference
        std::vector<float> f0((size_t)H * W), f1((size_t)H * W);
        auto widen = [&](const RawImage &im, std::vector<float> &f) {
            if (im.bpp == 1) for (size_t k = 0; k < f.size(); k++) f[k] = (float)im.px[k];
            else { const uint16_t *q = reinterpret_cast<const uint16_t *>(im.px.data()); for (size_t k = 0; k < f.size(); k++) f[k] = (float)q[k]; }
        };
        widen(i0, f0); widen(i1, f1);
        rc = mg ? mimc3_mgpu_set_images(mg, f0.data(), f1.data(), H, W) : mimc3_ctx_set_images(ctx, f0.data(), f1.data(), H, W);
    }
    if (rc) { fprintf(stderr, "%s\n", mimc3_last_error()); return leave(3); }
    lap("pair upload");

    std::vector<float> vx(N), vy(N), ex(N), ey(N), qual(N);
    std::vector<uint8_t> flag(N);
    mimc3_vmap_result r{};
    rc = mg ? mimc3_mgpu_vmap(mg, xy.data(), N, dt, &p, vx.data(), vy.data(), ex.data(), ey.data(), qual.data(), flag.data(), &r)
            : mimc3_vmap(ctx, xy.data(), N, dt, &p, vx.data(), vy.data(), ex.data(), ey.data(), qual.data(), flag.data(), &r);
    if (rc) {
        fprintf(stderr, "%s\n", mimc3_last_error());
        return leave(3);
    }
    lap("vmap (data path)");
    if (mg) printf("grid points sharded over %d GPU(s), work imbalance %.1f %%\n", (int)mimc3_mgpu_ndev(mg), 100.0 * mimc3_mgpu_last_imbalance(mg));
    // (no teardown on the way out: freeing the device buffers and the HIP runtime's exit handlers cost 50+ ms and the
    //  process is about to end -- the outputs are written, then the process leaves through _exit)
    printf("MPP=%f, grid spacing=%f, meter per spacing=%fm\nDimension of the vmap: %d by %d (mapy / mapx)\n", r.mpp, r.spacing_grid,
           r.meter_per_spacing, r.dimy, r.dimx);
    if (r.cp_status < 0) {                                                              // :246-252
        printf("Generating dummy vmap file.\n");
        FILE *f = fopen(f_tar.c_str(), "ab");
        if (f) fclose(f);
        return leave(-1);
    }
    printf("Measured offset: [%d, %d] pixels (i1-i0)\n", r.offset_cp[0], r.offset_cp[1]);

    // ---- outputs (:404-447)
    std::vector<double> gx(r.dimx), gy(r.dimy);
    for (int32_t c = 0; c < r.dimx; c++) gx[c] = xy[6 * (size_t)c];
    for (int32_t c = 0; c < r.dimy; c++) gy[c] = xy[6 * (size_t)c * r.dimx + 1];
    printf("Saving the output\n");
    bool ok = save_gma(base + "_x.GMA", gx.data(), 1, r.dimx) && save_gma(base + "_y.GMA", gy.data(), 1, r.dimy) &&
              save_gma(base + "_vx.GMA", vx.data(), r.dimy, r.dimx) && save_gma(base + "_vy.GMA", vy.data(), r.dimy, r.dimx) &&
              save_gma(base + "_ex.GMA", ex.data(), r.dimy, r.dimx) && save_gma(base + "_ey.GMA", ey.data(), r.dimy, r.dimx) &&
              save_gma(base + "_qual.GMA", qual.data(), r.dimy, r.dimx) && save_gma(base + "_flagcp.GMA", flag.data(), r.dimy, r.dimx);
    FILE *fm = fopen((base + "_meta.txt").c_str(), "w");
    if (fm) {
        fprintf(fm, "MIMC_version=%s\nname_i0=%s\nname_i1=%s\ncp_offset_int_u=%d\ncp_offset_int_v=%d\ncp_offset_subint_u=%f\ncp_offset_subint_v=%f\n",
                ver, argv[1], argv[2], r.offset_cp[0], r.offset_cp[1], r.cp_subint[0], r.cp_subint[1]);
        ok = fclose(fm) == 0 && ok;
    } else ok = false;
    if (!ok) { fprintf(stderr, "could not write the outputs under %s\n", argv[4]); return leave(4); }
    lap("outputs written");
    printf("Processing completed\n");
    return leave(0);
}
