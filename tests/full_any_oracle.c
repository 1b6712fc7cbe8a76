/* full_any_oracle.c -- the test-side oracle of the exhaustive search on ANY f32 pair (mimc3_match_ncc_full_any, include/mimc3_hip.h):
 * non-integral pixels, NaN and negative nulls.
 *
 * Test infrastructure only: compiled by tests/full_any_common.py into tests/_build with the flags tests/full_search_common.py uses
 * (-O3 -fno-tree-slp-vectorize -fopenmp -ffp-contract=off), and read through ctypes.
 *
 * The record, the local-maximum rule, the rank and the candidates are written again here as in tests/full_dn_oracle.c, statement by
 * statement (tests/test_full_any_cpu.py holds the two against each other on the integer classes).  New here:
 *   - the reference's TWO null rules, which differ on NaN: validity counts p < MIN_DN (MIMC_module.c:622, :631; a NaN is not counted),
 *     inclusion is a >= MIN_DN && b >= MIN_DN (:723; a NaN is excluded).  full_dn_oracle.c uses p < MIN_DN for both;
 *   - the pixel order of the sums is a parameter: order 0 is the reference's (:719-721, columns outer, rows inner, one accumulator per
 *     sum), order 1 runs the pixels backwards into four interleaved partial sums that are added at the end -- another order of the
 *     same additions, for the CPU check of the header's bound;
 *   - the tail is a function of a surface alone (tail_from_surface), which full_any calls on the surface it has summed.  snr_order 0
 *     adds the SNR's squares in k order (as the other oracles); 1 adds them as the device tail does: partial sum l takes the cells
 *     k = l, l + 64, ... in ascending order, then a pairwise tree over the 64 (s[l] += s[l ^ o], o = 1, 2, .. 32). */
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

/* record o[8], candidates (slot j of point g of n) and the local-maximum count of ONE point from its surface val[S * S] (k order);
 * lm: scratch, S * S ints */
static int tail_point(const float *val, int R, int shu, int shv, int npeaks, int snr_order, float *o, float *cand, int n, int g, int *lm)
{
    const int S = 2 * R + 1, NC = S * S;
    /* ---- the candidates: the local maxima, ranked by (NCC descending, k ascending) by repeated selection ---- */
    int nl = 0;
    for (int k = 0; k < NC; k++) {
        lm[k] = is_local_max(val, S, k / S, k % S);
        nl += lm[k];
    }
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
    /* ---- the record ---- */
    float bv = -INFINITY;
    int bk = -1;
    for (int k = 0; k < NC; k++)
        if (isfinite(val[k]) && val[k] > bv) { bv = val[k]; bk = k; }
    if (bk < 0) { store_status(o, -2.0f); return nl; }
    const int px = bk / S, py = bk % S, su = px - R, sv = py - R;
    if (su == -R || su == R || sv == -R || sv == R) { store_status(o, -4.0f); return nl; }
    double part[64];
    for (int l = 0; l < 64; l++) part[l] = 0.0;
    double s2 = 0.0;
    int cnt = 0;
    for (int k = 0; k < NC; k++) {
        const int x = k / S, y = k % S;
        if (!isfinite(val[k]) || (abs(x - px) <= 1 && abs(y - py) <= 1)) continue;
        s2 += (double)val[k] * (double)val[k];
        part[k & 63] += (double)val[k] * (double)val[k];
        cnt++;
    }
    if (snr_order) {
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
            double nx[64];
            for (int l = 0; l < 64; l++) nx[l] = part[l] + part[l ^ o2];
            for (int l = 0; l < 64; l++) part[l] = nx[l];
        }
        s2 = part[0];
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
    return nl;
}

/* The record and candidates of n points from given surfaces surf[n][S * S].  A point whose surface is all NaN AND whose refused[g] is
 * set (optional) is a status -3 point: (NaN, NaN, -3) everywhere.  Returns 0, -1 for npeaks outside 0..8. */
int tail_from_surface(const float *surf, const uint8_t *refused, int n, const int32_t *shift, int R, int npeaks, int snr_order,
                      float *out, float *cand, int32_t *nlm)
{
    const int S = 2 * R + 1, NC = S * S;
    if (npeaks < 0 || npeaks > 8) return -1;
    int *lm = (int *)malloc(sizeof(int) * NC);
    for (int g = 0; g < n; g++) {
        if (nlm) nlm[g] = 0;
        if (refused && refused[g]) {
            store_status(out + 8 * (size_t)g, -3.0f);
            store_slots(cand, n, g, 0, npeaks, -3.0f);
            continue;
        }
        const int shu = shift ? shift[2 * (size_t)g] : 0, shv = shift ? shift[2 * (size_t)g + 1] : 0;
        const int nl = tail_point(surf + (size_t)g * NC, R, shu, shv, npeaks, snr_order, out + 8 * (size_t)g, cand, n, g, lm);
        if (nlm) nlm[g] = nl;
    }
    free(lm);
    return 0;
}

/* Returns 0, or -2 if a chip leaves the image (the library refuses those), -1 for npeaks outside 0..8.
 *   order  0: the reference's pixel order; 1: backwards into four interleaved partial sums
 *   out    [n][8]          the record
 *   cand   [npeaks][n][3]  the candidates (not read when npeaks == 0)
 *   nlm    [n] (optional)  the number of local maxima of every point's surface (0 without a surface)
 *   surf   [n][S * S] (optional)  every point's surface in k order, NaN without one
 *   sums   [n][S * S][6] (optional)  every cell's n, sx, sy, sxx, syy, sxy as summed (0 without a surface): the CPU check of the bound */
int full_any(const float *i0, const float *i1, int H, int W, const double *xyuvav, int n, int off_u, int off_v,
             const int32_t *shift, int ocw, int R, int npeaks, int swap, int order, float *out, float *cand, int32_t *nlm, float *surf,
             double *sums, int nthreads)
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
            if (sums) for (int k = 0; k < 6 * NC; k++) sums[(size_t)g * 6 * NC + k] = 0.0;
            const int u0 = (int)xyuvav[6 * (size_t)g + 2], v0 = (int)xyuvav[6 * (size_t)g + 3];
            const int shu = shift ? shift[2 * (size_t)g] : 0, shv = shift ? shift[2 * (size_t)g + 1] : 0;
            const int cu = u0 + off_u + shu, cv = v0 + off_v + shv;
            /* chip a[y][x], search box b[y][x] = B at (cu - R - ocw + x, cv - R - ocw + y), 0 outside the image.
             * Validity (:622, :631): p < MIN_DN -- false on a NaN */
            int bad_chip = 0, bad_box = 0;
            for (int y = 0; y < cw; y++)
                for (int x = 0; x < cw; x++) {
                    const float q = A[(size_t)(v0 - ocw + y) * W + (u0 - ocw + x)];
                    a[y * cw + x] = q;
                    if (q < MIN_DN) bad_chip++;
                }
            for (int y = 0; y < SB; y++)
                for (int x = 0; x < SB; x++) {
                    const int pu = cu - R - ocw + x, pv = cv - R - ocw + y;
                    const float q = (pu >= 0 && pu < W && pv >= 0 && pv < H) ? B[(size_t)pv * W + pu] : 0.0f;
                    b[y * SB + x] = q;
                    if (q < MIN_DN) bad_box++;
                }
            const float max_ratio = 0.8f;
            if ((float)bad_chip / (float)(cw * cw) > max_ratio || (float)bad_box / (float)(SB * SB) > max_ratio) {
                store_status(o, -3.0f);
                store_slots(cand, n, g, 0, npeaks, -3.0f);
                continue;
            }
            /* every cell: k = (su + R) S + (sv + R), tile cell (x, y) = (su + R, sv + R).  Inclusion (:723): a >= MIN_DN && b >= MIN_DN
             * -- false on a NaN */
            for (int x = 0; x < S; x++)
                for (int y = 0; y < S; y++) {
                    double dn = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
                    if (order == 0) {
                        for (int c = 0; c < cw; c++)            /* cnt3: columns outer */
                            for (int r = 0; r < cw; r++) {      /* cnt4: rows inner */
                                const float pa = a[r * cw + c], pb = b[(y + r) * SB + (x + c)];
                                if (pa >= MIN_DN && pb >= MIN_DN) {
                                    const float paa = pa * pa, pbb = pb * pb, pab = pa * pb;      /* the reference's f32 products */
                                    dn += 1.0; sx += (double)pa; sy += (double)pb;
                                    sxx += (double)paa; syy += (double)pbb; sxy += (double)pab;
                                }
                            }
                    } else {
                        double px[4] = {0, 0, 0, 0}, py[4] = {0, 0, 0, 0}, pxx[4] = {0, 0, 0, 0}, pyy[4] = {0, 0, 0, 0}, pxy[4] = {0, 0, 0, 0};
                        for (int t = cw * cw - 1; t >= 0; t--) {
                            const int r = t / cw, c = t % cw;
                            const float pa = a[r * cw + c], pb = b[(y + r) * SB + (x + c)];
                            if (pa >= MIN_DN && pb >= MIN_DN) {
                                const float paa = pa * pa, pbb = pb * pb, pab = pa * pb;
                                dn += 1.0; px[t & 3] += (double)pa; py[t & 3] += (double)pb;
                                pxx[t & 3] += (double)paa; pyy[t & 3] += (double)pbb; pxy[t & 3] += (double)pab;
                            }
                        }
                        sx = (px[0] + px[1]) + (px[2] + px[3]); sy = (py[0] + py[1]) + (py[2] + py[3]);
                        sxx = (pxx[0] + pxx[1]) + (pxx[2] + pxx[3]); syy = (pyy[0] + pyy[1]) + (pyy[2] + pyy[3]);
                        sxy = (pxy[0] + pxy[1]) + (pxy[2] + pxy[3]);
                    }
                    val[x * S + y] = (float)((dn * sxy - sx * sy) / sqrt((dn * sxx - sx * sx) * (dn * syy - sy * sy)));
                    if (sums) {
                        double *q = sums + ((size_t)g * NC + (size_t)(x * S + y)) * 6;
                        q[0] = dn; q[1] = sx; q[2] = sy; q[3] = sxx; q[4] = syy; q[5] = sxy;
                    }
                }
            if (surf) for (int k = 0; k < NC; k++) surf[(size_t)g * NC + k] = val[k];
            const int nl = tail_point(val, R, shu, shv, npeaks, 0, o, cand, n, g, lm);
            if (nlm) nlm[g] = nl;
        }
        free(a); free(b); free(val); free(lm);
    }
    return 0;
}
