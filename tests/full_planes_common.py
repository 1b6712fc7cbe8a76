"""Test infrastructure of the exhaustive search on scaled-integer pairs (mimc3_match_ncc_full_planes): the fixtures the CPU and GPU
tests share, and a float restatement of the reference's cell for the scale-invariance test."""
import numpy as np

from full_multi_common import STATUS_R, status_case

PLANES_OCW = (7, 16, 30, 40)
PLANES_R = (1, 7, 15)


def dn12_case(ocw, null_frac, radius, dimx=5, dimy=4):
    """full_multi_common.parity_case's pair and grid, times 16: 12-bit DN below 4096 (nulls stay 0).  -> (case, i0, i1, a-priori shift)"""
    from full_multi_common import parity_case
    c, shift = parity_case(ocw, null_frac, radius, dimx=dimx, dimy=dimy)
    i0, i1 = np.ascontiguousarray(c.i0 * 16, np.float32), np.ascontiguousarray(c.i1 * 16, np.float32)
    assert i0.max() < 4096 and i0.max() > 255 and (i0 == np.rint(i0)).all()
    return c, i0, i1, shift


def status_case12():
    """full_multi_common.status_case times 16, with two more points: 6 has a null in its chip alone, 7 one in its chip and one in its
    box.  -> (i0, i1, xyuvav); ocw 7, R = STATUS_R"""
    i0, i1, xy = status_case()
    i0 = i0 * 16; i1 = i1 * 16
    xy = np.concatenate([xy, np.zeros((2, 6))])
    xy[6, 2:4] = [90, 40]
    xy[7, 2:4] = [60, 100]
    i0[40, 90] = 0
    i0[100, 60] = 0
    i1[95, 55] = 0
    return np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32), xy


def null_sides(i0, i1, xy, ocw, radius, offset=(0, 0)):
    """Per point: (nulls in the chip, nulls in the search box, box pixels outside the image counted as nulls)."""
    H, W = i0.shape
    res = []
    for g in range(xy.shape[0]):
        u, v = int(xy[g, 2]), int(xy[g, 3])
        chip = i0[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1]
        h = ocw + radius
        cu, cv = u + offset[0], v + offset[1]
        box = np.zeros((2 * h + 1, 2 * h + 1), np.float32)
        y0, y1, x0, x1 = max(cv - h, 0), min(cv + h + 1, H), max(cu - h, 0), min(cu + h + 1, W)
        box[y0 - (cv - h):y1 - (cv - h), x0 - (cu - h):x1 - (cu - h)] = i1[y0:y1, x0:x1]
        res.append((int((chip == 0).sum()), int((box == 0).sum())))
    return res


def ncc_cell_f32(a, b):
    """The reference's cell (MIMC_module.c:719-734, as ncc_at of oracle/mimc3_oracle.c) on float pixels: null exclusion at MIN_DN, f32
    products, f64 sums in pixel order, the f64 formula, cast to f32.  a, b: float32 [cw][cw]."""
    a = np.asarray(a, np.float32).ravel(); b = np.asarray(b, np.float32).ravel()
    thr = 1e-10
    n = 0.0; sx = sy = sxx = syy = sxy = np.float64(0.0)
    for pa, pb in zip(a, b):
        if float(pa) < thr or float(pb) < thr:
            continue
        n += 1.0
        sx += np.float64(pa); sy += np.float64(pb)
        sxx += np.float64(np.float32(pa * pa)); syy += np.float64(np.float32(pb * pb)); sxy += np.float64(np.float32(pa * pb))
    n = np.float64(n)
    with np.errstate(all="ignore"):
        return np.float32((n * sxy - sx * sy) / np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy)))


def surface_f32(i0, i1, u0, v0, ocw, radius):
    """ncc_cell_f32 of every offset of one point (search centre uv0) -> float32[S * S] in k order (u outer)."""
    S = 2 * radius + 1
    chip = i0[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1]
    val = np.empty(S * S, np.float32)
    for x in range(S):
        for y in range(S):
            cu, cv = u0 + x - radius, v0 + y - radius
            val[x * S + y] = ncc_cell_f32(chip, i1[cv - ocw:cv + ocw + 1, cu - ocw:cu + ocw + 1])
    return val
