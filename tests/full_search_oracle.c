/* full_search_oracle.c -- the test-side oracle of the exhaustive-search entry (mimc3_match_ncc_full, include/mimc3_hip.h).
 *
 * Test infrastructure only: compiled by tests/full_search_common.py into tests/_build with the flags the repository's oracle uses
 * (-O3 -fno-tree-slp-vectorize -fopenmp -ffp-contract=off: no fused multiply-add, scalar f32 expressions as written -- the
 * reference's x86-64 build never contracts either), and read through ctypes.
 *
 * For 8-bit pairs (integers 0..255 held as f32, 0 = null).  Every cell comes from exact integer sums (int64) and the reference's f64
 * formula (MIMC_module.c:719-734, as oracle/mimc3_oracle.c's ncc_at: there the f32 products of 8-bit pixels and their f64 sums are
 * exact integers too); the peak, border and validity rules and the 3x3 fit follow the header's text line by line, the fit in the
 * reference's float/double order (:757-788).  The SNR sum runs in k order. */
#include <math.h>
#include <omp.h>
#include <stdint.h>
#include <stdlib.h>

static void store_status(float *o, float status)
{
    const float nanv = nanf("");
    o[0] = nanv; o[1] = nanv; o[2] = status;
    for (int i = 3; i < 8; i++) o[i] = nanv;
}

/* returns 0, or -2 if a chip leaves the image (the library refuses those); peak_k (optional) gets the arg-max k or -1 */
int full_search(const float *i0, const float *i1, int H, int W, const double *xyuvav, int n, int off_u, int off_v,
                const int32_t *shift, int ocw, int R, int swap, float *out, int32_t *peak_k, int nthreads)
{
    const float *A = swap ? i1 : i0, *B = swap ? i0 : i1;
    const int cw = 2 * ocw + 1, S = 2 * R + 1, SB = 2 * R + cw, NC = S * S;
    for (int g = 0; g < n; g++) {
        const int u0 = (int)xyuvav[6 * (size_t)g + 2], v0 = (int)xyuvav[6 * (size_t)g + 3];
        if (u0 - ocw < 0 || u0 + ocw >= W || v0 - ocw < 0 || v0 + ocw >= H) return -2;
    }
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel
    {
        int *a = (int *)malloc(sizeof(int) * cw * cw), *b = (int *)malloc(sizeof(int) * SB * SB);
        float *val = (float *)malloc(sizeof(float) * NC);
#pragma omp for schedule(dynamic, 16)
        for (int g = 0; g < n; g++) {
            float *o = out + 8 * (size_t)g;
            if (peak_k) peak_k[g] = -1;
            const int u0 = (int)xyuvav[6 * (size_t)g + 2], v0 = (int)xyuvav[6 * (size_t)g + 3];
            const int shu = shift ? shift[2 * (size_t)g] : 0, shv = shift ? shift[2 * (size_t)g + 1] : 0;
            const int cu = u0 + off_u + shu, cv = v0 + off_v + shv;
            /* chip a[y][x] (extract_refchip), search box b[y][x] = B at (cu - R - ocw + x, cv - R - ocw + y), 0 outside the image */
            int bad_chip = 0, bad_box = 0;
            for (int y = 0; y < cw; y++)
                for (int x = 0; x < cw; x++) {
                    const int q = (int)A[(size_t)(v0 - ocw + y) * W + (u0 - ocw + x)];
                    a[y * cw + x] = q;
                    bad_chip += q == 0;
                }
            for (int y = 0; y < SB; y++)
                for (int x = 0; x < SB; x++) {
                    const int pu = cu - R - ocw + x, pv = cv - R - ocw + y;
                    const int q = (pu >= 0 && pu < W && pv >= 0 && pv < H) ? (int)B[(size_t)pv * W + pu] : 0;
                    b[y * SB + x] = q;
                    bad_box += q == 0;
                }
            const float max_ratio = 0.8f;
            if ((float)bad_chip / (float)(cw * cw) > max_ratio || (float)bad_box / (float)(SB * SB) > max_ratio) {
                store_status(o, -3.0f);
                continue;
            }
            /* every cell: k = (su + R) S + (sv + R), tile cell (x, y) = (su + R, sv + R) */
            for (int x = 0; x < S; x++)
                for (int y = 0; y < S; y++) {
                    int64_t nn = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
                    for (int r = 0; r < cw; r++)
                        for (int c = 0; c < cw; c++) {
                            const int64_t pa = a[r * cw + c], pb = b[(y + r) * SB + (x + c)];
                            if (pa != 0 && pb != 0) { nn++; sx += pa; sy += pb; sxx += pa * pa; syy += pb * pb; sxy += pa * pb; }
                        }
                    const double dn = (double)nn, dsx = (double)sx, dsy = (double)sy;
                    val[x * S + y] = (float)((dn * (double)sxy - dsx * dsy) /
                                             sqrt((dn * (double)sxx - dsx * dsx) * (dn * (double)syy - dsy * dsy)));
                }
            float bv = -INFINITY;
            int bk = -1;
            for (int k = 0; k < NC; k++)
                if (isfinite(val[k]) && val[k] > bv) { bv = val[k]; bk = k; }
            if (peak_k) peak_k[g] = bk;
            if (bk < 0) { store_status(o, -2.0f); continue; }
            const int px = bk / S, py = bk % S, su = px - R, sv = py - R;
            if (su == -R || su == R || sv == -R || sv == R) { store_status(o, -4.0f); continue; }
            double s2 = 0.0;
            int cnt = 0;
            for (int k = 0; k < NC; k++) {
                const int x = k / S, y = k % S;
                if (!isfinite(val[k]) || (abs(x - px) <= 1 && abs(y - py) <= 1)) continue;
                s2 += (double)val[k] * (double)val[k];
                cnt++;
            }
            float n9[9];     /* n9[3 r + c] = cell (px - 1 + c, py - 1 + r), as ncc9 (:759-767) */
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) n9[3 * r + c] = val[(px - 1 + c) * S + (py - 1 + r)];
            double cp[6];
            cp[0] = 6 * n9[0] - 12 * n9[1] + 6 * n9[2] + 6 * n9[3] - 12 * n9[4] + 6 * n9[5] + 6 * n9[6] - 12 * n9[7] + 6 * n9[8];
            cp[1] = 9 * n9[0] - 9 * n9[2] - 9 * n9[6] + 9 * n9[8];
            cp[2] = 6 * n9[0] + 6 * n9[1] + 6 * n9[2] - 12 * n9[3] - 12 * n9[4] - 12 * n9[5] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
            cp[3] = -6 * n9[0] + 6 * n9[2] - 6 * n9[3] + 6 * n9[5] - 6 * n9[6] + 6 * n9[8];
            cp[4] = -6 * n9[0] - 6 * n9[1] - 6 * n9[2] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
            cp[5] = -4 * n9[0] + 8 * n9[1] - 4 * n9[2] + 8 * n9[3] + 20 * n9[4] + 8 * n9[5] - 4 * n9[6] + 8 * n9[7] - 4 * n9[8];
            for (int i = 0; i < 6; i++) cp[i] /= 36;
            float uv[2];
            uv[0] = -2 * cp[2] * cp[3] + cp[1] * cp[4];
            uv[1] = -2 * cp[0] * cp[4] + cp[1] * cp[3];
            uv[0] /= 4 * cp[0] * cp[2] - cp[1] * cp[1];
            uv[1] /= 4 * cp[0] * cp[2] - cp[1] * cp[1];
            uv[0] += (float)(su + shu);
            uv[1] += (float)(sv + shv);
            const double det = 4 * cp[0] * cp[2] - cp[1] * cp[1];
            const double xs = (-2 * cp[2] * cp[3] + cp[1] * cp[4]) / det, ys = (-2 * cp[0] * cp[4] + cp[1] * cp[3]) / det;
            const double fit = cp[0] * xs * xs + cp[1] * xs * ys + cp[2] * ys * ys + cp[3] * xs + cp[4] * ys + cp[5];
            o[0] = uv[0]; o[1] = uv[1]; o[2] = bv; o[3] = (float)fit;
            o[4] = cnt > 0 ? (float)(((double)bv * (double)bv) / (s2 / (double)cnt)) : nanf("");
            o[5] = (float)(2 * cp[0]); o[6] = (float)cp[1]; o[7] = (float)(2 * cp[2]);
        }
        free(a); free(b); free(val);
    }
    return 0;
}
