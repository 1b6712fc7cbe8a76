"""CPU: the interface of the exhaustive search on scaled-integer pairs (mimc3_match_ncc_full_planes) and the scale invariance its
definition rests on: the reference's cell on float pixels q / 8 equals the integer oracle's cell on q bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from full_planes_common import null_sides, status_case12, surface_f32, STATUS_R
from full_search_common import full_search
from full_multi_common import full_multi, surface_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mimc3_match_ncc_full_planes", "mimc3_match_ncc_full_planes_dev")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared in mimc3_hip.h"
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"


@pytest.mark.parametrize("kind", ["laplacian", "dn12"])
def test_scale_invariance_of_the_cell(kind):
    """q < 4096 with nulls; the float pixels are q / 8 (Laplacian-like: multiples of 1/8) or q (12-bit DN) on one side and q / 8 on the
    other.  Every cell of the float surface equals the integer cell on q (full_multi_common.surface_py: int64 sums, the f64 formula)
    bit for bit, NaN positions included; its first finite maximum in k order is tests/full_search_oracle.c's arg-max cell, and its
    value (or -4 on the border) that oracle's ncc_peak, bit for bit."""
    rng = np.random.default_rng(5 if kind == "laplacian" else 6)
    H = W = 64
    q0 = rng.integers(1, 4096, (H, W)).astype(np.float32)
    q1 = np.roll(q0, (1, -2), axis=(0, 1)) + rng.integers(-40, 41, (H, W)).astype(np.float32)
    q1 = np.clip(q1, 1, 4095).astype(np.float32)
    q0[rng.random((H, W)) < 0.03] = 0
    q1[rng.random((H, W)) < 0.03] = 0
    q1[20:26, 30:40] = 0
    f0 = q0 / np.float32(8) if kind == "laplacian" else q0
    f1 = q1 / np.float32(8)
    ocw, radius = 7, 3
    xy = np.zeros((4, 6))
    xy[:, 2:4] = [[20, 20], [32, 28], [40, 40], [25, 42]]
    out, peak = full_search(q0, q1, xy, (0, 0), ocw, radius, with_peak=True)
    assert (peak >= 0).all()
    for g in range(xy.shape[0]):
        u0, v0 = int(xy[g, 2]), int(xy[g, 3])
        val = surface_f32(f0, f1, u0, v0, ocw, radius)
        ints = surface_py(q0, q1, u0, v0, u0, v0, ocw, radius).reshape(-1)          # [x][y]: k order
        assert np.isnan(val).sum() == np.isnan(ints).sum()
        assert np.array_equal(np.isnan(val), np.isnan(ints)) and np.array_equal(np.nan_to_num(val).view(np.uint32), np.nan_to_num(ints).view(np.uint32))
        fin = np.isfinite(val)
        k = int(np.flatnonzero(fin & (val == val[fin].max()))[0])
        assert k == peak[g]
        S = 2 * radius + 1
        border = k // S in (0, S - 1) or k % S in (0, S - 1)
        want = np.float32(-4.0) if border else val[k]
        assert np.array_equal(np.array([want]).view(np.uint32), out[g, 2:3].view(np.uint32)), (g, val[k], out[g, 2])
    # the integer oracle is scale-blind too: q and 8 q give the same records
    out8 = full_search(q0 * 8, q1 * 8, xy, (0, 0), ocw, radius)
    assert np.array_equal(out.view(np.uint32), out8.view(np.uint32))


def test_status_case_holds_every_class():
    """The GPU null / status fixture, on the oracle alone: statuses -2, -3, -4; chip nulls only, box nulls only, both; a point with
    fewer than npeaks local maxima."""
    i0, i1, xy = status_case12()
    assert i0.max() < 4096 and i0.max() > 255
    out, cand, nlm = full_multi(i0, i1, xy, (0, 0), 7, STATUS_R, 4, with_counts=True)
    st = out[:, 2]
    assert (st == -2).any() and (st == -3).any() and (st == -4).any()
    sides = null_sides(i0, i1, xy, 7, STATUS_R)
    assert any(c > 0 and b == 0 for c, b in sides) and any(c == 0 and b > 0 for c, b in sides) and any(c > 0 and b > 0 for c, b in sides)
    assert any(c == 0 and b == 0 for c, b in sides)
    assert ((nlm < 4) & (st != -3)).any()
