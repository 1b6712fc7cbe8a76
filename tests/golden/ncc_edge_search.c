/* ncc_edge_search.c -- the search behind tests/golden/make_ncc_edge_fixtures.py (fixture generation only; no test runs it).
 *
 * One NCC cell: a chip a[i] and the window pixels under it b[i] (8-bit values, 0 = null; a pair counts when both are non-zero).
 * The search rewrites the window pixels at three of the given positions, each to a value within +-delta of its own, and returns the
 * first candidate (in a fixed order) whose cell value lies at a wanted distance from an f32 rounding midpoint:
 *
 *   Qd = (n sxy - sx sy) / sqrt((n sxx - sx^2)(n syy - sy^2))   (exact integer sums, IEEE f64 operations, as the reference)
 *   d  = (bits(Qd) & (2^29 - 1)) - 2^28                           (f64 ulps from the midpoint between two f32 neighbours)
 *
 * Candidates update sy, syy and sxy incrementally; n, sx and sxx do not change (both values of a rewritten pair are non-zero). */
#include <math.h>
#include <stdint.h>
#include <string.h>

static int64_t dist_of(int64_t n, int64_t sx, int64_t sxx, int64_t sy, int64_t syy, int64_t sxy)
{
    const double dn = (double)n, dsx = (double)sx, dsy = (double)sy;
    const double q = (dn * (double)sxy - dsx * dsy) / sqrt((dn * (double)sxx - dsx * dsx) * (dn * (double)syy - dsy * dsy));
    uint64_t bits;
    memcpy(&bits, &q, 8);
    return (int64_t)(bits & ((1ull << 29) - 1)) - (1ll << 28);
}

/* the cell's d as it stands */
int64_t edge_cell_d(const int32_t *a, const int32_t *b, int np)
{
    int64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int i = 0; i < np; i++)
        if (a[i] != 0 && b[i] != 0) { n++; sx += a[i]; sy += b[i]; sxx += (int64_t)a[i] * a[i]; syy += (int64_t)b[i] * b[i]; sxy += (int64_t)a[i] * b[i]; }
    return dist_of(n, sx, sxx, sy, syy, sxy);
}

/* Triples (i < j < k) of pos[] in lexicographic order, values ascending within each.  Accepts d in [dlo, dhi] (and, with abs_range,
 * also in [-dhi, -dlo]); skips the first `skip` hits; gives up after max_cand candidates.  Returns 1 and out[6] = (p_i, p_j, p_k,
 * v_i, v_j, v_k, d as out[6]) on a hit, 0 otherwise.  pos[] must name pixels whose a and b are both non-zero. */
int edge_search(const int32_t *a, const int32_t *b, int np, const int32_t *pos, int npos, int delta, int64_t dlo, int64_t dhi,
                int abs_range, int skip, int64_t max_cand, int64_t *out)
{
    int64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0, cand = 0;
    for (int i = 0; i < np; i++)
        if (a[i] != 0 && b[i] != 0) { n++; sx += a[i]; sy += b[i]; sxx += (int64_t)a[i] * a[i]; syy += (int64_t)b[i] * b[i]; sxy += (int64_t)a[i] * b[i]; }
    for (int i = 0; i < npos; i++)
        for (int j = i + 1; j < npos; j++)
            for (int k = j + 1; k < npos; k++) {
                const int pi = pos[i], pj = pos[j], pk = pos[k];
                const int64_t ai = a[pi], aj = a[pj], ak = a[pk], bi = b[pi], bj = b[pj], bk = b[pk];
                const int64_t sy0 = sy - bi - bj - bk, syy0 = syy - bi * bi - bj * bj - bk * bk, sxy0 = sxy - ai * bi - aj * bj - ak * bk;
                const int lo_i = bi - delta < 1 ? 1 : (int)bi - delta, hi_i = bi + delta > 255 ? 255 : (int)bi + delta;
                const int lo_j = bj - delta < 1 ? 1 : (int)bj - delta, hi_j = bj + delta > 255 ? 255 : (int)bj + delta;
                const int lo_k = bk - delta < 1 ? 1 : (int)bk - delta, hi_k = bk + delta > 255 ? 255 : (int)bk + delta;
                for (int64_t vi = lo_i; vi <= hi_i; vi++)
                    for (int64_t vj = lo_j; vj <= hi_j; vj++) {
                        const int64_t sy1 = sy0 + vi + vj, syy1 = syy0 + vi * vi + vj * vj, sxy1 = sxy0 + ai * vi + aj * vj;
                        for (int64_t vk = lo_k; vk <= hi_k; vk++) {
                            const int64_t d = dist_of(n, sx, sxx, sy1 + vk, syy1 + vk * vk, sxy1 + ak * vk);
                            if ((d >= dlo && d <= dhi) || (abs_range && d >= -dhi && d <= -dlo)) {
                                if (skip-- <= 0) {
                                    out[0] = pi; out[1] = pj; out[2] = pk; out[3] = vi; out[4] = vj; out[5] = vk; out[6] = d;
                                    return 1;
                                }
                            }
                        }
                        cand += hi_k - lo_k + 1;
                        if (cand > max_cand) return 0;
                    }
            }
    return 0;
}
