// cli_io.h -- what the two command lines (MIMC3_hip, MIMC3_hip_offsets) share: the reference program's file-name timestamps and
// dt (MIMC_misc.c), its TIFF reader (GMA.c) kept at the raw DN, and the .GMA container (GMA.c).  Included once per program.
#ifndef MIMC3_CLI_IO_H
#define MIMC3_CLI_IO_H
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <tiffio.h>
#include "../../../include/mimc3_hip.h"

namespace {

bool leap(int y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }          // MIMC_misc.c:9-25

double datenum(const char *s)                                                       // MIMC_misc.c:27-119
{
    char buf[8];
    auto field = [&](int at, int len) { std::memset(buf, 0, sizeof buf); std::memcpy(buf, s + at, len); return buf; };
    const int y = atoi(field(0, 4));
    const int m = atoi(field(4, 2));
    const int d = atoi(field(6, 2));
    const double H = atof(field(8, 2));
    const double M = atof(field(10, 2));
    const double S = atof(field(12, 2));
    double off = 0.0;
    for (int k = 0; k < y; k++) off += leap(k) ? 366.0 : 365.0;
    static const int acc_n[12] = {0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334};
    static const int acc_l[12] = {0, 31, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335};
    const int *acc = leap(y) ? acc_l : acc_n;
    off += (double)acc[m - 1] + (double)d + H / 24.0 + M / 1440.0 + S / 86400.0;
    return off;
}

bool timestamp_of(const char *path, char out[15])                                   // MIMC_misc.c:133-153
{
    const char *slash = std::strrchr(path, '/');
    if (!slash || std::strlen(slash + 1) < 14) return false;      // the reference reads garbage here; this refuses
    std::memcpy(out, slash + 1, 14);
    out[14] = '\0';
    for (int i = 0; i < 14; i++)
        if (out[i] < '0' || out[i] > '9') return false;
    return true;
}

// GMA_float_load_tiff (GMA.c:246-316): scanline reader; bytes per pixel = scanline size / width, 1 -> u8, 2 -> u16.
// The reference widens to float32 on the host (:288-310); here the RAW DN is kept (scanlines are read straight into
// the buffer that crosses PCIe) and the widening runs on the device (mimc3_ctx_set_images_u8/_u16).
// Anything the reference's reader would misread (1/4-bit, multi-sample, 32-bit) is refused instead.
struct RawImage {
    std::vector<unsigned char> px;      // H * W * bpp bytes, row-major
    int32_t H = 0, W = 0, bpp = 0;
};
bool load_tiff(const char *path, RawImage &img)
{
    TIFF *tif = TIFFOpen(path, "r");
    if (!tif) return false;
    uint32_t h = 0, w = 0;
    uint16_t bits = 0, spp = 1;
    TIFFGetField(tif, TIFFTAG_IMAGELENGTH, &h);
    TIFFGetField(tif, TIFFTAG_IMAGEWIDTH, &w);
    TIFFGetFieldDefaulted(tif, TIFFTAG_BITSPERSAMPLE, &bits);
    TIFFGetFieldDefaulted(tif, TIFFTAG_SAMPLESPERPIXEL, &spp);
    const tsize_t scan = TIFFScanlineSize(tif);
    const int bpp = bits / 8;
    if (h == 0 || w == 0 || scan <= 0 || (bits != 8 && bits != 16) || spp != 1 || (size_t)scan != (size_t)w * bpp) {
        fprintf(stderr, "%s: only single-sample 8- or 16-bit images are supported (bits=%d, samples=%d)\n", path, (int)bits, (int)spp);
        TIFFClose(tif);
        return false;
    }
    img.px.resize((size_t)h * w * bpp);
    for (uint32_t r = 0; r < h; r++)
        if (TIFFReadScanline(tif, img.px.data() + (size_t)r * scan, r, 0) < 0) { TIFFClose(tif); return false; }
    TIFFClose(tif);
    img.H = (int32_t)h; img.W = (int32_t)w; img.bpp = bpp;
    printf("Loading TIFF - row=%d, col=%d, bytes per pixel=%d\n", img.H, (int)scan, bpp);
    return true;
}

// .GMA container (GMA.c:168-244, :319-424): int32 rows, int32 cols, row-major payload
bool load_gma_double(const char *path, std::vector<double> &v, int32_t &rows, int32_t &cols)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    bool ok = fread(&rows, 4, 1, f) == 1 && fread(&cols, 4, 1, f) == 1 && rows > 0 && cols > 0;
    if (ok) { v.resize((size_t)rows * cols); ok = fread(v.data(), 8, v.size(), f) == v.size(); }
    fclose(f);
    return ok;
}
template <class T> bool save_gma(const std::string &path, const T *p, int32_t rows, int32_t cols)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = fwrite(&rows, 4, 1, f) == 1 && fwrite(&cols, 4, 1, f) == 1 && fwrite(p, sizeof(T), (size_t)rows * cols, f) == (size_t)rows * cols;
    return fclose(f) == 0 && ok;
}

// the reference program's parameters and filter kernels (MIMC_main.c:134-194); MIMC3_CP_SEED pins the control-point shuffle
mimc3_vmap_params reference_vmap_params()
{
    static const float k_dx[3] = {-1, 0, 1}, k_dy[3] = {-1, 0, 1};
    static const float k_lap[9] = {-1.0 / 8, -1.0 / 8, -1.0 / 8, -1.0 / 8, 1.0, -1.0 / 8, -1.0 / 8, -1.0 / 8, -1.0 / 8};
    mimc3_vmap_params p{};
    p.vec_ocw[0] = 7; p.vec_ocw[1] = 15; p.vec_ocw[2] = 30; p.vec_ocw[3] = 40;
    p.aw_cre = 10.0f; p.aw_sf = 1.8f;
    p.radius_neighbor_dpf1 = 1000 / 300; p.radius_neighbor_ps = 5.0f;
    p.num_cp_max = 500; p.num_cp_min = 50; p.ratio_cp = 0.03f; p.thres_spd_cp = 10;
    p.kernel[0] = k_dx; p.kdim[0][0] = 1; p.kdim[0][1] = 3;
    p.kernel[1] = k_dy; p.kdim[1][0] = 3; p.kdim[1][1] = 1;
    p.kernel[2] = k_lap; p.kdim[2][0] = 3; p.kdim[2][1] = 3;
    const char *seed = getenv("MIMC3_CP_SEED");
    p.cp_seed = seed ? atoll(seed) : -1;
    p.qm_max_sweeps = 101;
    return p;
}

}  // namespace

#endif
