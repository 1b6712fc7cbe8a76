"""Test infrastructure: the rounding-edge NCC fixtures (tests/golden/ncc_edge_*.npz, written by tests/golden/make_ncc_edge_fixtures.py).

Each fixture is one 8-bit image pair with points on a grid, one target cell per point, and the point's own pivot list.  A target cell's
f64 NCC value Qd (the reference's formula on exact integer sums) lies d f64 ulps from an f32 rounding midpoint,
d = (bits(Qd) & (2^29 - 1)) - 2^28, so a result off by a few f64 ulps before its f32 rounding lands on the other f32 neighbour.

Columns of `targets` (int64): point, su, sv, role, form, d.
  (su, sv)  the cell, as an offset of its window's centre from uv0 + offset (the peak of every point is at (0, 0))
  role      0 the peak, 1..8 the neighbour NEIGHBOURS[role - 1] of the peak
  form      0 clean, 1 window nulls inside the target cell's box, 2 chip nulls
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
FORMS = ("clean", "window nulls", "chip nulls")
T_POINT, T_SU, T_SV, T_ROLE, T_FORM, T_D = range(6)


def fixture_paths():
    return sorted(os.path.join(GOLDEN, f) for f in os.listdir(GOLDEN) if f.startswith("ncc_edge_") and f.endswith(".npz"))


def load(path):
    z = np.load(path)
    d = {k: z[k] for k in z.files}
    d["i0"] = d["i0"].astype(np.float32)
    d["i1"] = d["i1"].astype(np.float32)
    d["ocw"] = int(d["ocw"]); d["radius"] = int(d["radius"])
    d["name"] = os.path.basename(path)
    return d


def cell_sums(i0, i1, xyuvav, offset, ocw, g, su, sv):
    """Exact integer sums (n, sx, sxx, sy, syy, sxy) of point g's cell (su, sv): chip of i0 at uv0, window of i1 at uv0 + offset + s."""
    u0, v0 = int(xyuvav[g, 2]), int(xyuvav[g, 3])
    uc, vc = u0 + int(offset[0]) + su, v0 + int(offset[1]) + sv
    a = i0[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1].astype(np.int64)
    b = i1[vc - ocw:vc + ocw + 1, uc - ocw:uc + ocw + 1].astype(np.int64)
    m = (a != 0) & (b != 0)
    a = np.where(m, a, 0); b = np.where(m, b, 0)
    return int(m.sum()), int(a.sum()), int((a * a).sum()), int(b.sum()), int((b * b).sum()), int((a * b).sum())


def qd(sums):
    """The reference's f64 value of a cell from its exact sums, IEEE f64 operations in the reference's order."""
    n, sx, sxx, sy, syy, sxy = (np.float64(v) for v in sums)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (n * sxy - sx * sy) / np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy))


def midpoint_distance(q):
    bits = int(np.float64(q).view(np.uint64))
    return (bits & ((1 << 29) - 1)) - (1 << 28)


def surface(i0, i1, xyuvav, offset, ocw, g, radius):
    """f64 surface Qd[x][y] over (su, sv) = (x - R, y - R), x, y in 0..2R (k = x (2R + 1) + y order when flattened)."""
    S = 2 * radius + 1
    out = np.empty((S, S), np.float64)
    for x in range(S):
        for y in range(S):
            out[x, y] = qd(cell_sums(i0, i1, xyuvav, offset, ocw, g, x - radius, y - radius))
    return out


def fit(n9, su, sv):
    """The reference's 3x3 fit (:757-788) in numpy scalars: f32 expressions widened to f64, the numerators stored to f32 before the f64
    division, the quotient stored to f32, then the cell offset added in f32.  n9[3 r + c] = cell (su - 1 + c, sv - 1 + r)."""
    n = [np.float32(v) for v in n9]
    f = np.float32
    e = [f(6) * n[0] - f(12) * n[1] + f(6) * n[2] + f(6) * n[3] - f(12) * n[4] + f(6) * n[5] + f(6) * n[6] - f(12) * n[7] + f(6) * n[8],
         f(9) * n[0] - f(9) * n[2] - f(9) * n[6] + f(9) * n[8],
         f(6) * n[0] + f(6) * n[1] + f(6) * n[2] - f(12) * n[3] - f(12) * n[4] - f(12) * n[5] + f(6) * n[6] + f(6) * n[7] + f(6) * n[8],
         -f(6) * n[0] + f(6) * n[2] - f(6) * n[3] + f(6) * n[5] - f(6) * n[6] + f(6) * n[8],
         -f(6) * n[0] - f(6) * n[1] - f(6) * n[2] + f(6) * n[6] + f(6) * n[7] + f(6) * n[8]]
    cp = [np.float64(v) / 36 for v in e]
    den = 4 * cp[0] * cp[2] - cp[1] * cp[1]
    q0 = np.float32(-2 * cp[2] * cp[3] + cp[1] * cp[4])
    q1 = np.float32(-2 * cp[0] * cp[4] + cp[1] * cp[3])
    return np.float32(np.float64(q0) / den) + np.float32(su), np.float32(np.float64(q1) / den) + np.float32(sv)
