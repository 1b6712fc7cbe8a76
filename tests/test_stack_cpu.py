"""CPU: the interface of NCC stacking (mimc3_stack_*) and its definition on the host: NumpyStack (tests/stack_common.py) over the
surfaces of the float oracle (tests/full_any_oracle.c) -- a stack of one layer is the search itself, what min_count does, and the
reason for the feature: on a noisy series the stack misplaces fewer points than any of its layers."""
import ctypes
import os
import re

import numpy as np

from conftest import assert_bits_equal
from full_any_common import full_any
from full_fb_common import FB_OFFSET, class_pair, fb_points
from mimc3_amd.api import STACK_CHUNK
from stack_common import (SERIES_NOISE_DN, SERIES_OCW, SERIES_PAIRS, SERIES_R, SERIES_TRUTH, SHAPES, NumpyStack, misplaced, refused_of,
                          series_pairs, series_points)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"mimc3_stack_begin": 4, "mimc3_stack_add": 6, "mimc3_stack_add_dev": 8, "mimc3_stack_add_surfaces": 4,
        "mimc3_stack_add_surfaces_dev": 5, "mimc3_stack_finish": 7, "mimc3_stack_finish_dev": 8, "mimc3_stack_info": 4}


def test_symbols_declared_and_exported():
    """The entries exist, with the argument counts of the header (and the Python binding's), and the chunk is the header's."""
    from mimc3_amd import api
    hdr = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    assert int(re.search(r"#define\s+MIMC3_STACK_CHUNK\s+(\d+)", hdr).group(1)) == STACK_CHUNK == 65536
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s, nargs in SYMS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, f"{s} is not declared in mimc3_hip.h"
        assert len(m.group(1).split(",")) == nargs, s
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"
        assert len(getattr(api._lib, s).argtypes) == nargs, s
    for name in ("stack_begin", "stack_add", "stack_add_dev", "stack_add_surfaces", "stack_add_surfaces_dev", "stack_finish",
                 "stack_finish_dev", "stack_info"):
        assert callable(getattr(api.Context, name)), name


def test_one_layer_is_the_search():
    """A stack of one layer at min_count 1: (float)((double)v / 1.0) == v, so the mean is the layer and the result is the oracle's
    own record (its SNR in the oracle's order of additions: the tail is then the oracle's, statement by statement) and candidates."""
    from full_any_common import tail_from_surface
    i0, i1, _ = class_pair("float")
    for ocw, radius in SHAPES:
        xy, shift = fb_points(ocw=ocw, radius=radius)
        for sh in (shift, None):
            rec, cand, surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 8, shift=sh)
            st = NumpyStack(xy.shape[0], radius, sh).add(surf, refused_of(rec))
            assert_bits_equal(st.mean(1), surf, f"ocw {ocw} R {radius}: mean of one layer")
            assert np.array_equal(st.lay, (~refused_of(rec)).astype(np.uint16))
            got_rec, got_cand = tail_from_surface(st.mean(1), st.shift, radius, 8, refused=st.lay == 0)
            assert_bits_equal(got_rec, rec, f"ocw {ocw} R {radius} shift {sh is not None}: record")
            assert_bits_equal(got_cand, cand, f"ocw {ocw} R {radius} shift {sh is not None}: candidates")
            # the device tail's SNR order changes column 4 at most
            dev_rec, dev_cand, _, _ = st.finish(8)
            assert_bits_equal(np.delete(dev_rec, 4, axis=1), np.delete(rec, 4, axis=1), "record but the SNR")
            assert_bits_equal(dev_cand, cand, "candidates")


def test_min_count_semantics():
    """Three crafted layers at R 1: a cell's mean is over its finite values alone; below min_count it is NaN; Inf is no value; a point
    every layer refuses gets -3 whatever its cells hold; f64 sums in layer order, one rounding to f32."""
    nan, inf = np.nan, np.inf
    a = np.array([[0.1, 0.2, 0.1, 0.2, 0.9, 0.2, 0.1, 0.2, 0.1], [0.5] * 9], np.float32)
    b = np.array([[nan, 0.4, 0.1, inf, 0.7, 0.2, -inf, 0.2, 0.1], [0.5] * 9], np.float32)
    c = np.array([[nan, nan, 0.4, nan, 0.5, 0.2, nan, 0.2, nan], [0.5] * 9], np.float32)
    st = NumpyStack(2, 1)
    for layer in (a, b, c):
        st.add(layer, refused=[False, True])
    assert st.cnt[0].tolist() == [1, 2, 3, 1, 3, 3, 1, 3, 2] and st.lay.tolist() == [3, 0] and st.layers == 3
    m1, m2, m3 = st.mean(1), st.mean(2), st.mean(3)
    assert np.isfinite(m1[0]).all() and m1[0, 0] == np.float32(0.1) and m1[0, 3] == np.float32(0.2)
    assert np.isnan(m2[0, [0, 3, 6]]).all() and np.isfinite(m2[0, [1, 2, 4, 5, 7, 8]]).all()
    assert np.isfinite(m3[0]).tolist() == [False, False, True, False, True, True, False, True, False]
    want = np.float32((np.float64(np.float32(0.9)) + np.float64(np.float32(0.7)) + np.float64(np.float32(0.5))) / 3.0)
    assert m3[0, 4] == want and m1[0, 4] == want
    for mc in (1, 2, 3):
        rec, cand, lay, _ = st.finish(2, mc)
        assert rec[1, 2] == -3 and np.isnan(np.delete(rec[1], 2)).all() and (cand[:, 1, 2] == -3).all()
        assert rec[0, 2] == want                              # the centre cell is the peak: a fit whose NaN neighbours show in (du, dv)
        assert np.isfinite(rec[0, :2]).all() == (mc == 1)
    rec, _, _, _ = st.finish(0, 4)
    assert rec[0, 2] == -2                                    # no cell reaches min_count: no finite cell


def test_the_stack_beats_its_layers_on_a_noisy_series():
    """SERIES_PAIRS = 6 pairs (synth.make_pair, 160 x 160, 8-bit) that moved by the same (3, -2) px, each with its own texture and its
    own +-SERIES_NOISE_DN = +-100 DN of uniform noise on image 1; 60 points, ocw 7, R 4.  A point is misplaced when it has no fit or
    its fit lies more than 0.5 px from the truth.  The layers misplace 28, 14, 29, 26, 23 and 20 of the 60 points; the stack of the
    six misplaces 1 (point 56, whose true peak lies on the border of its box: status -4 in every layer and in the stack)."""
    xy, shift = series_points()
    st = NumpyStack(xy.shape[0], SERIES_R, shift)
    per_layer = []
    for i0, i1 in series_pairs():
        rec, _, surf, _ = full_any(i0, i1, xy, FB_OFFSET, SERIES_OCW, SERIES_R, 0, shift=shift)
        per_layer.append(int(misplaced(rec, SERIES_TRUTH).sum()))
        st.add(surf, refused_of(rec))
    rec = st.finish()[0]
    stacked = int(misplaced(rec, SERIES_TRUTH).sum())
    print(f"noise +-{SERIES_NOISE_DN} DN: misplaced per layer {per_layer}, stack of {SERIES_PAIRS}: {stacked}")
    assert len(per_layer) >= 5 and min(per_layer) > 0, per_layer
    assert stacked < min(per_layer), (stacked, per_layer)
    assert per_layer == [28, 14, 29, 26, 23, 20] and stacked == 1 and rec[56, 2] == -4
