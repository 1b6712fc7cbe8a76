"""CPU: the interface of the forward-backward consistency check (mimc3_match_ncc_full_fb) and its definition on the host: fb_chain
(tests/full_fb_common.py) driven by the C oracle of the exhaustive search (tests/full_dn_oracle.c) on the shared fixture -- what the
back-match tells apart, every status -- and the seed and compose arithmetic at their edges."""
import ctypes
import os
import re

import numpy as np

from conftest import assert_bits_equal
from full_fb_common import (FB_OCW, FB_OFFSET, FB_R, fb_areas, fb_chain, fb_compose, fb_pair, fb_points, fb_seed, oracle_search, rint_f32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"mimc3_match_ncc_full_fb": 12, "mimc3_match_ncc_full_fb_dev": 14}


def test_symbols_declared_and_exported():
    """The two entries exist, with the argument counts of the header (and the Python binding's)."""
    from mimc3_amd import api
    hdr = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s, nargs in SYMS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, f"{s} is not declared in mimc3_hip.h"
        assert len(m.group(1).split(",")) == nargs, s
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"
        assert len(getattr(api._lib, s).argtypes) == nargs, s
    assert callable(api.Context.match_ncc_full_fb) and callable(api.Context.match_ncc_full_fb_dev)


def test_chain_on_the_oracle():
    """The shared fixture through the oracle chain: the back-match confirms the shifted area and rejects the noise area, and every
    status occurs.  The counts are exact: the oracle is deterministic integer arithmetic."""
    i0, i1 = fb_pair()
    H, W = i0.shape
    xy, shift = fb_points()
    out, cand, fb, why = fb_chain(oracle_search(i0, i1), xy, FB_OFFSET, FB_OCW, FB_R, H, W, npeaks=3, shift=shift)
    n = xy.shape[0]
    assert out.shape == (n, 8) and cand.shape == (3, n, 3) and fb.shape == (4, n, 4) and why.shape == (4, n)
    shifted, noise = fb_areas(xy)
    err, st = fb[0, :, 3], fb[0, :, 2]
    with np.errstate(invalid="ignore"):
        good, bad = shifted & (err < 0.25), noise & (err > 1)
    print(f"shifted area: {int(shifted.sum())} points, {int(good.sum())} with err < 0.25; noise area: {int(noise.sum())} points, "
          f"{int(bad.sum())} with err > 1; plane-0 statuses {sorted(set(st[st < -1].tolist()))}")
    assert int(shifted.sum()) == 28 and int(noise.sum()) == 24
    assert int(good.sum()) == 25                  # every shifted-area point but 56 (-5), 57 and 58 (-6); the largest err is 0.077
    # of the 24 noise points 9 have no forward fit (-5) and 4 no backward fit (-4); of the other 11, 5 come back elsewhere (err 2.2 to
    # 4.9) and 6 come back (err 0.11 to 0.39): the backward search sees the pixel pairs of the forward peak again, so a noise peak
    # is reciprocal wherever it is also the largest cell of the backward box -- err is a criterion beside NCC (0.10 to 0.19 here), not
    # in its place
    assert int(bad.sum()) == 5
    # where the forward match is right, the backward match undoes it
    fwd_ok = shifted & (np.abs(out[:, 0] - 2) < 0.25) & (np.abs(out[:, 1] + 1) < 0.25)
    assert np.array_equal(good, fwd_ok & (st >= -1))
    # the statuses
    assert out[56, 2] == -4 and st[56] == -5 and np.isnan(fb[0, 56, [0, 1, 3]]).all()
    assert out[57, 2] >= -1 and st[57] == -6 and st[58] == -6 and np.isnan(fb[0, 57, [0, 1, 3]]).all()
    assert (st[noise] == -4).any(), "a backward peak on the border passes through"
    through = st == -4
    assert (why[0][through] == 0).all() and (out[through, 2] >= -1).all() and np.isnan(fb[0][through][:, [0, 1, 3]]).all()
    assert set(np.unique(why).tolist()) == {0, 5, 6}
    # planes: candidate 0 is the record where the record has a fit; an empty slot is -5
    fit = out[:, 2] >= -1
    assert_bits_equal(fb[1][fit], fb[0][fit], "plane 1 vs plane 0 where the record has a fit")
    empty = cand[:, :, 2] < -1
    assert empty.any() and (fb[1:][empty][:, 2] == -5).all()
    # the border point's interior local maxima are still matched back
    assert cand[0, 56, 2] >= -1 and why[1, 56] == 0
    # without candidates: plane 0 alone, the same bytes
    out0, none, fb0, _ = fb_chain(oracle_search(i0, i1), xy, FB_OFFSET, FB_OCW, FB_R, H, W, npeaks=0, shift=shift)
    assert none is None
    assert_bits_equal(out0, out, "record, npeaks 0")
    assert_bits_equal(fb0[0], fb[0], "plane 0, npeaks 0")


def test_rintf_halves_go_to_even():
    x = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 2.4999998, 2.5000002, -2.5000002, 8388607.5, 0.0, -0.0], np.float32)
    assert rint_f32(x).tolist() == [0, 2, 2, 4, 0, -2, -2, -4, 2, 3, -3, 8388608, 0, 0]


def test_seed_edges():
    H = W = 100
    ocw = 7
    xy = np.zeros((8, 6))
    xy[:, 2:4] = [[50.9, 50.2]] * 6 + [[90, 50], [50, 9]]
    du = np.array([[2.5, 3.5, -2.5, -3.5, np.nan, np.float32(2.0 ** 30), 1.25, 0.0]], np.float32)
    dv = np.array([[-0.5, 0.5, 1.5, -1.5, 1.0, 0.0, 0.0, -2.5]], np.float32)
    xy2, sh2, why = fb_seed(xy, (1, -1), du, dv, ocw, H, W)
    assert why.tolist() == [0, 0, 0, 0, 5, 6, 0, 6]
    # m = (int)uv0 + offset + r;  r: halves to even, both parities, negative halves
    assert xy2[:4, 2:4].tolist() == [[53, 49], [55, 49], [49, 51], [47, 47]]
    assert sh2[:4].tolist() == [[-2, 0], [-4, 0], [2, -2], [4, 2]]
    assert xy2[6, 2:4].tolist() == [92, 49] and xy2[6, 2] + ocw == W - 1          # the last column a chip may reach
    # rows that are not searched: a chip no kernel reads, shift 0; the other columns are the point's
    assert xy2[[4, 5, 7], 2:4].tolist() == [[-1, -1]] * 3 and sh2[[4, 5, 7]].tolist() == [[0, 0]] * 3
    assert np.array_equal(xy2[:, [0, 1, 4, 5]], xy[:, [0, 1, 4, 5]])
    # one more column to the right leaves the image
    assert fb_seed(xy[6:7], (1, -1), np.array([[1.5]], np.float32), np.array([[0.0]], np.float32), ocw, H, W)[2].tolist() == [6]
    # an infinite fit is no fit
    assert fb_seed(xy[:1], (0, 0), np.array([[np.inf]], np.float32), np.array([[0.0]], np.float32), ocw, H, W)[2].tolist() == [5]


def test_compose_edges():
    du = np.array([[2.25, 2.25, 2.25, 2.25, np.nan, 3.0]], np.float32)
    dv = np.array([[-1.5, -1.5, -1.5, -1.5, np.nan, 4.0]], np.float32)
    back = np.full((6, 8), np.nan, np.float32)
    back[0, :3] = [-2.25, 1.5, 0.9]               # reciprocal: err 0
    back[1, :3] = [np.nan, np.nan, -4]            # the backward search's own status passes through
    back[2, :3] = [np.inf, 0.0, 0.5]              # a degenerate backward fit: no err
    back[3, :3] = [0.75, -2.5, 0.25]              # err = hypot(3, -4)
    back[5, :3] = [np.float32(1e-3), np.float32(-1e-3), 0.7]
    why = np.array([0, 0, 0, 0, 5, 0], np.uint8)
    fb = fb_compose(du, dv, back, why)[0]
    assert fb[0].tolist() == [-2.25, 1.5, np.float32(0.9), 0.0]
    assert fb[1, 2] == -4 and np.isnan(fb[1, [0, 1, 3]]).all()
    assert np.isinf(fb[2, 0]) and fb[2, 2] == 0.5 and np.isnan(fb[2, 3])
    assert fb[3, 3] == 5.0
    assert fb[4, 2] == -5 and np.isnan(fb[4, [0, 1, 3]]).all()
    a, b = np.float64(np.float32(3.0)) + np.float64(np.float32(1e-3)), np.float64(np.float32(4.0)) + np.float64(np.float32(-1e-3))
    assert fb[5, 3] == np.float32(np.hypot(a, b))                        # the sums in f64, rounded once at the end
    assert fb_compose(du[:, :1], dv[:, :1], back[:1], np.array([6], np.uint8))[0, 0, 2] == -6
