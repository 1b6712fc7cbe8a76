/* full_dn_oracle.c -- the test-side oracle of the exhaustive search on float pixels (mimc3_match_ncc_full_dn, include/mimc3_hip.h).
 *
 * Test infrastructure only: compiled by tests/full_dn_common.py into tests/_build with the flags tests/full_search_common.py uses
 * (-O3 -fno-tree-slp-vectorize -fopenmp -ffp-contract=off: no fused multiply-add, scalar f32 expressions as written), and read
 * through ctypes.
 *
 * For any f32 pair (16-bit DN and its filtered forms are what the tests give it).  The validity rule, the [N][8] record, the
 * local-maximum rule, the rank and the candidates are written again here as in tests/full_search_oracle.c and
 * tests/full_multi_oracle.c, statement by statement, so that on 8-bit and 12-bit pairs the three agree bit for bit
 * (tests/test_full_dn_cpu.py holds them against each other).  New here: the cell reads the float pixels and forms the reference's
 * sums as the reference does (MIMC_module.c:719-734; tests/full_planes_common.py's ncc_cell_f32) -- null exclusion at MIN_DN, f32
 * pixel products that round above 2^24, f64 sums in pixel order, the f64 formula, cast to f32.  With exact != 0 the products are
 * taken exactly instead (f64 products of f32 pixels, the arithmetic of the two integer oracles): the tests use that to show that a
 * fixture tells the two apart. */
#include <math.h>
#include <omp.h>
#include <stdint.h>
#include <stdlib.h>

#define MIN_DN 1e-10

static void store_status(float *o, float status)
{
    const float nanv = nanf("");
    o[0] = nanv; o[1] = nanv; o[2] = status;
    for (int i = 3; i < 8; i++) o[i] = nanv;
}

static void store_slots(float *cand, int n, int g, int j0, int npeaks, float status)
{
    const float nanv = nanf("");
    for (int j = j0; j < npeaks; j++) {
        float *q = cand + 3 * ((size_t)j * (size_t)n + (size_t)g);
        q[0] = nanv; q[1] = nanv; q[2] = status;
    }
}

/* the reference's 3x3 fit (:757-788) around cell (px, py) of val[x * S + y]: the sub-cell offset before the cell's own is added */
static void fit9(const float *val, int S, int px, int py, double cp[6], float uv[2])
{
    float n9[9];     /* n9[3 r + c] = cell (px - 1 + c, py - 1 + r), as ncc9 (:759-767) */
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) n9[3 * r + c] = val[(px - 1 + c) * S + (py - 1 + r)];
    cp[0] = 6 * n9[0] - 12 * n9[1] + 6 * n9[2] + 6 * n9[3] - 12 * n9[4] + 6 * n9[5] + 6 * n9[6] - 12 * n9[7] + 6 * n9[8];
    cp[1] = 9 * n9[0] - 9 * n9[2] - 9 * n9[6] + 9 * n9[8];
    cp[2] = 6 * n9[0] + 6 * n9[1] + 6 * n9[2] - 12 * n9[3] - 12 * n9[4] - 12 * n9[5] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
    cp[3] = -6 * n9[0] + 6 * n9[2] - 6 * n9[3] + 6 * n9[5] - 6 * n9[6] + 6 * n9[8];
    cp[4] = -6 * n9[0] - 6 * n9[1] - 6 * n9[2] + 6 * n9[6] + 6 * n9[7] + 6 * n9[8];
    cp[5] = -4 * n9[0] + 8 * n9[1] - 4 * n9[2] + 8 * n9[3] + 20 * n9[4] + 8 * n9[5] - 4 * n9[6] + 8 * n9[7] - 4 * n9[8];
    for (int i = 0; i < 6; i++) cp[i] /= 36;
    uv[0] = -2 * cp[2] * cp[3] + cp[1] * cp[4];
    uv[1] = -2 * cp[0] * cp[4] + cp[1] * cp[3];
    uv[0] /= 4 * cp[0] * cp[2] - cp[1] * cp[1];
    uv[1] /= 4 * cp[0] * cp[2] - cp[1] * cp[1];
}

/* is cell (x, y) a local maximum of val[x * S + y] (S = 2R + 1)?  The header's three conditions. */
static int is_local_max(const float *val, int S, int x, int y)
{
    if (x < 1 || x > S - 2 || y < 1 || y > S - 2) return 0;           /* |su| < R and |sv| < R */
    const float v = val[x * S + y];
    const int k = x * S + y;
    if (!isfinite(v)) return 0;
    for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
            if (dx == 0 && dy == 0) continue;
            const int kt = (x + dx) * S + (y + dy);
            const float t = val[kt];
            if (!isfinite(t)) continue;
            if (v > t) continue;
            if (v == t && k < kt) continue;
            return 0;
        }
    return 1;
}

/* Returns 0, or -2 if a chip leaves the image (the library refuses those), -1 for npeaks outside 0..8.
 *   out    [n][8]          the record of mimc3_match_ncc_full
 *   cand   [npeaks][n][3]  the candidates (not read when npeaks == 0)
 *   nlm    [n] (optional)  the number of local maxima of every point's surface (0 without a surface)
 *   surf   [n][S * S] (optional)  every point's surface in k order, NaN without one */
int full_dn(const float *i0, const float *i1, int H, int W, const double *xyuvav, int n, int off_u, int off_v,
            const int32_t *shift, int ocw, int R, int npeaks, int swap, int exact, float *out, float *cand, int32_t *nlm, float *surf,
            int nthreads)
{
    const float *A = swap ? i1 : i0, *B = swap ? i0 : i1;
    const int cw = 2 * ocw + 1, S = 2 * R + 1, SB = 2 * R + cw, NC = S * S;
    if (npeaks < 0 || npeaks > 8) return -1;
    for (int g = 0; g < n; g++) {
        const int u0 = (int)xyuvav[6 * (size_t)g + 2], v0 = (int)xyuvav[6 * (size_t)g + 3];
        if (u0 - ocw < 0 || u0 + ocw >= W || v0 - ocw < 0 || v0 + ocw >= H) return -2;
    }
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel
    {
        float *a = (float *)malloc(sizeof(float) * cw * cw), *b = (float *)malloc(sizeof(float) * SB * SB);
        float *val = (float *)malloc(sizeof(float) * NC);
        int *lm = (int *)malloc(sizeof(int) * NC);
#pragma omp for schedule(dynamic, 16)
        for (int g = 0; g < n; g++) {
            float *o = out + 8 * (size_t)g;
            if (nlm) nlm[g] = 0;
            if (surf) for (int k = 0; k < NC; k++) surf[(size_t)g * NC + k] = nanf("");
            const int u0 = (int)xyuvav[6 * (size_t)g + 2], v0 = (int)xyuvav[6 * (size_t)g + 3];
            const int shu = shift ? shift[2 * (size_t)g] : 0, shv = shift ? shift[2 * (size_t)g + 1] : 0;
            const int cu = u0 + off_u + shu, cv = v0 + off_v + shv;
            /* chip a[y][x] (extract_refchip), search box b[y][x] = B at (cu - R - ocw + x, cv - R - ocw + y), 0 outside the image */
            int bad_chip = 0, bad_box = 0;
            for (int y = 0; y < cw; y++)
                for (int x = 0; x < cw; x++) {
                    const float q = A[(size_t)(v0 - ocw + y) * W + (u0 - ocw + x)];
                    a[y * cw + x] = q;
                    bad_chip += (double)q < MIN_DN;
                }
            for (int y = 0; y < SB; y++)
                for (int x = 0; x < SB; x++) {
                    const int pu = cu - R - ocw + x, pv = cv - R - ocw + y;
                    const float q = (pu >= 0 && pu < W && pv >= 0 && pv < H) ? B[(size_t)pv * W + pu] : 0.0f;
                    b[y * SB + x] = q;
                    bad_box += (double)q < MIN_DN;
                }
            const float max_ratio = 0.8f;
            if ((float)bad_chip / (float)(cw * cw) > max_ratio || (float)bad_box / (float)(SB * SB) > max_ratio) {
                store_status(o, -3.0f);
                store_slots(cand, n, g, 0, npeaks, -3.0f);
                continue;
            }
            /* every cell: k = (su + R) S + (sv + R), tile cell (x, y) = (su + R, sv + R) */
            for (int x = 0; x < S; x++)
                for (int y = 0; y < S; y++) {
                    double dn = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
                    for (int r = 0; r < cw; r++)
                        for (int c = 0; c < cw; c++) {
                            const float pa = a[r * cw + c], pb = b[(y + r) * SB + (x + c)];
                            if ((double)pa < MIN_DN || (double)pb < MIN_DN) continue;
                            dn += 1.0; sx += (double)pa; sy += (double)pb;
                            if (exact) {
                                sxx += (double)pa * (double)pa; syy += (double)pb * (double)pb; sxy += (double)pa * (double)pb;
                            } else {
                                const float paa = pa * pa, pbb = pb * pb, pab = pa * pb;      /* the reference's f32 products */
                                sxx += (double)paa; syy += (double)pbb; sxy += (double)pab;
                            }
                        }
                    val[x * S + y] = (float)((dn * sxy - sx * sy) / sqrt((dn * sxx - sx * sx) * (dn * syy - sy * sy)));
                }
            if (surf) for (int k = 0; k < NC; k++) surf[(size_t)g * NC + k] = val[k];
            /* ---- the candidates: the local maxima, ranked by (NCC descending, k ascending) by repeated selection ---- */
            int nl = 0;
            for (int k = 0; k < NC; k++) {
                lm[k] = is_local_max(val, S, k / S, k % S);
                nl += lm[k];
            }
            if (nlm) nlm[g] = nl;
            for (int j = 0; j < npeaks; j++) {
                int bk = -1;
                for (int k = 0; k < NC; k++)
                    if (lm[k] && (bk < 0 || val[k] > val[bk])) bk = k;          /* ascending k: the first of equals stays */
                if (bk < 0) {
                    store_slots(cand, n, g, j, npeaks, -2.0f);
                    break;
                }
                lm[bk] = 0;
                const int px = bk / S, py = bk % S;
                double cp[6];
                float uv[2];
                fit9(val, S, px, py, cp, uv);
                uv[0] += (float)(px - R + shu);
                uv[1] += (float)(py - R + shv);
                float *q = cand + 3 * ((size_t)j * (size_t)n + (size_t)g);
                q[0] = uv[0]; q[1] = uv[1]; q[2] = val[bk];
            }
            /* ---- the record, as tests/full_search_oracle.c ---- */
            float bv = -INFINITY;
            int bk = -1;
            for (int k = 0; k < NC; k++)
                if (isfinite(val[k]) && val[k] > bv) { bv = val[k]; bk = k; }
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
            double cp[6];
            float uv[2];
            fit9(val, S, px, py, cp, uv);
            uv[0] += (float)(su + shu);
            uv[1] += (float)(sv + shv);
            const double det = 4 * cp[0] * cp[2] - cp[1] * cp[1];
            const double xs = (-2 * cp[2] * cp[3] + cp[1] * cp[4]) / det, ys = (-2 * cp[0] * cp[4] + cp[1] * cp[3]) / det;
            const double fit = cp[0] * xs * xs + cp[1] * xs * ys + cp[2] * ys * ys + cp[3] * xs + cp[4] * ys + cp[5];
            o[0] = uv[0]; o[1] = uv[1]; o[2] = bv; o[3] = (float)fit;
            o[4] = cnt > 0 ? (float)(((double)bv * (double)bv) / (s2 / (double)cnt)) : nanf("");
            o[5] = (float)(2 * cp[0]); o[6] = (float)cp[1]; o[7] = (float)(2 * cp[2]);
        }
        free(a); free(b); free(val); free(lm);
    }
    return 0;
}
