"""CPU: the interface of the scaled and weighted layers of NCC stacking (mimc3_stack_add_scaled and its kin) and their definition on
the host: NumpyScaledStack (tests/stack_scaled_common.py) over the surfaces of the float oracle -- the layer radius against brute force,
the two consequences the header states (scale 1 / weight 1 is the old add; one power-of-two weight everywhere is the unweighted mean), a
zero-weight tap on a NaN row, and the reason for the feature: a series over six time baselines, which the unscaled stack destroys."""
import ctypes
import os
import re

import numpy as np

from conftest import assert_bits_equal
from full_any_common import full_any
from full_fb_common import FB_OFFSET, class_pair, fb_points
from stack_common import SHAPES, NumpyStack, misplaced, refused_of
from stack_scaled_common import (SCALED_COUNTS, SCALED_MOTION, SCALED_NOISE_DN, SCALED_OCW, SCALED_R, NumpyScaledStack, axis_taps, layer_radius,
                                 layer_shift, layer_truth, resample, scaled_series_pairs, scaled_series_points)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"mimc3_stack_layer_radius": 2, "mimc3_stack_layer_shift": 3, "mimc3_stack_weighted": 1, "mimc3_stack_add_scaled": 9,
        "mimc3_stack_add_scaled_dev": 11, "mimc3_stack_add_surfaces_scaled": 7, "mimc3_stack_add_surfaces_scaled_dev": 8}
SCALES = (1, 2, 3, 0.5, 1.5, 1 / 3, 0.7, 2.5, 47 / 15)


def test_symbols_declared_and_exported():
    """The entries exist, with the argument counts of the header (and the Python binding's)."""
    from mimc3_amd import api
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mimc3_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s, nargs in SYMS.items():
        m = re.search(r"\bint(?:32_t)?\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, f"{s} is not declared in mimc3_hip.h"
        assert len(m.group(1).split(",")) == nargs, s
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"
        assert len(getattr(api._lib, s).argtypes) == nargs, s
    for name in ("stack_layer_shift", "stack_weighted", "stack_add_scaled", "stack_add_scaled_dev", "stack_add_surfaces_scaled",
                 "stack_add_surfaces_scaled_dev"):
        assert callable(getattr(api.Context, name)), name
    assert callable(api.stack_layer_radius)


def test_layer_radius_is_the_library_s():
    """mimc3_stack_layer_radius needs no device: the formula, and 0 for what no stack takes"""
    from mimc3_amd import api
    for s in SCALES + (2.0 ** -6, 64.0):
        for R in (1, 4, 15, 47):
            assert api.stack_layer_radius(R, s) == layer_radius(R, s), (R, s)
    assert [api.stack_layer_radius(4, s) for s in (1, 2, 0.5, 3, 1.5)] == [4, 9, 3, 13, 7]
    for R, s in ((0, 1.0), (48, 1.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, 128.0), (4, 2.0 ** -7), (4, float("inf"))):
        assert api.stack_layer_radius(R, s) == 0, (R, s)


def taps_inside(shifts, R, Rl, s, both):
    """bool per shift: the taps of every cell lie inside the layer of radius Rl -- those that are read (floor(pu), and floor(pu) + 1 where
    its weight is not zero), or with `both` the second tap whether it is read or not (one axis is the whole story: the axes are
    independent and alike)"""
    sh = np.asarray(shifts, np.int32)
    a, j = axis_taps(sh, layer_shift(sh, s), R, Rl, s)
    return ((j >= 0) & (j + (np.ones_like(j) if both else a != 0) <= 2 * Rl)).all(axis=1)


def test_layer_radius_against_brute_force():
    """At mimc3_stack_layer_radius every tap that is read lies inside for every shift in -9..9 (scale != 1: the unread ones too), and
    at one less some tap of some shift does not (scale != 1).  There both taps are counted, as in the header's argument for the formula:
    where pu is an integer (every cell of an integral scale) the second tap has weight zero and is never read, so such a layer would be
    served by one less -- the formula does not single those scales out."""
    shifts = np.arange(-9, 10)
    for s in SCALES:
        for R in (1, 4, 15):
            Rl = layer_radius(R, s)
            assert taps_inside(shifts, R, Rl, s, both=False).all(), (s, R, Rl)
            if s != 1:
                assert taps_inside(shifts, R, Rl, s, both=True).all(), (s, R, Rl)
                assert not taps_inside(shifts, R, Rl - 1, s, both=True).all(), (s, R, Rl)
            else:
                assert Rl == R and not taps_inside(shifts, R, Rl - 1, s, both=False).any()


def test_scale_one_weight_one_is_the_old_add():
    """s == 1, w == 1, Rl == R: every cell is one tap with value (double)v -- NumpyStack's bytes, and no wsum"""
    i0, i1, _ = class_pair("float")
    for ocw, radius in SHAPES[:2]:
        xy, shift = fb_points(ocw=ocw, radius=radius)
        rec, _, surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 0, shift=shift)
        extra = np.random.default_rng(radius).random(surf.shape).astype(np.float32)
        extra[3, 5], extra[4, 0] = np.nan, np.inf
        old, new = NumpyStack(xy.shape[0], radius, shift), NumpyScaledStack(xy.shape[0], radius, shift)
        for layer, ref in ((surf, refused_of(rec)), (extra, None)):
            old.add(layer, ref)
            new.add_scaled(layer, radius, 1.0, 1.0, ref)
        value, read, taps = resample(surf, radius, shift, radius, 1.0)
        assert read.all() and (taps == 1).all() and np.array_equal(layer_shift(shift, 1.0), shift)
        assert_bits_equal(value.astype(np.float32), surf, "value == (double)v")
        assert not new.weighted
        assert old.sum.tobytes() == new.sum.tobytes() and old.cnt.tobytes() == new.cnt.tobytes() and old.lay.tobytes() == new.lay.tobytes()
        for a, b in zip(old.finish(3, 2), new.finish(3, 2)):
            assert a.tobytes() == b.tobytes()


def test_one_power_of_two_weight_is_the_unweighted_mean():
    """Weight 2 on every layer: sum and wsum are twice the unweighted sum and cnt, exactly -- the mean's bytes do not change"""
    radius = 4
    xy, shift = fb_points(ocw=7, radius=radius)
    rng = np.random.default_rng(11)
    plain, heavy = NumpyScaledStack(xy.shape[0], radius, shift), NumpyScaledStack(xy.shape[0], radius, shift)
    for s in (0.5, 1.5, 2.0):
        Rl = layer_radius(radius, s) - (1 if s == 2.0 else 0)    # (one layer too small: cells without a count)
        layer = (rng.random((xy.shape[0], (2 * Rl + 1) ** 2)) - 0.4).astype(np.float32)
        layer[rng.random(layer.shape) < 0.02] = np.nan
        ref = np.arange(xy.shape[0]) % 7 == 0
        plain.add_scaled(layer, Rl, s, 1.0, ref)
        heavy.add_scaled(layer, Rl, s, 2.0, ref)
    assert heavy.weighted and not plain.weighted
    assert np.array_equal(heavy.sum, 2 * plain.sum) and np.array_equal(heavy.wsum, 2.0 * plain.cnt) and np.array_equal(heavy.cnt, plain.cnt)
    assert (plain.cnt < 3).any() and (plain.cnt == 3).any()
    for mc in (1, 3):
        assert_bits_equal(heavy.mean(mc), plain.mean(mc), f"min_count {mc}")
        for a, b in zip(heavy.finish(3, mc), plain.finish(3, mc)):
            assert a.tobytes() == b.tobytes()
    # unequal weights: (x + 3.5 y) / 4.5, the product and the sum and the quotient each rounded once; the lazy wsum starts from cnt
    x, y = rng.random((xy.shape[0], 81)).astype(np.float32), rng.random((xy.shape[0], 81)).astype(np.float32)
    other = NumpyScaledStack(xy.shape[0], radius, shift).add(x).add_scaled(y, radius, 1.0, 3.5)
    assert (other.wsum == 4.5).all() and (other.cnt == 2).all()
    assert_bits_equal(other.mean(2), ((x.astype(np.float64) + 3.5 * y.astype(np.float64)) / 4.5).astype(np.float32), "weights 1 and 3.5")


def test_a_zero_weight_tap_is_not_read():
    """Scale 2, shift 0, R 1, Rl 3: stack cell su lands on layer row 3 + 2 su exactly (au == 0), so rows 0, 2, 4 and 6 are never
    read: NaN there changes nothing.  Scale 0.5: su = +-1 reads two rows (au == 0.5) and the NaN row shows."""
    Rl, Sl = 3, 7
    L = (np.arange(Sl * Sl, dtype=np.float32) / 64).reshape(1, Sl, Sl)
    holes = L.copy()
    holes[0, [0, 2, 4, 6], :] = np.nan
    holes[0, :, [0, 2, 4, 6]] = np.nan
    st = NumpyScaledStack(1, 1).add_scaled(holes.reshape(1, -1), Rl, 2.0)
    assert (st.cnt == 1).all()
    assert st.sum.reshape(3, 3).tolist() == L[0, 1::2, 1::2].astype(np.float64).tolist()
    value, read, taps = resample(holes.reshape(1, -1), Rl, np.zeros((1, 2), np.int32), 1, 2.0)
    assert read.all() and (taps == 1).all()
    # one radius less: rows 1 and 5 of the layer become rows 0 and 4 of a 5 x 5 one -- the outer cells' single tap lies outside
    st = NumpyScaledStack(1, 1).add_scaled(np.ones((1, 9), np.float32), 1, 2.0)
    assert st.cnt.reshape(3, 3).tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    # scale 0.5 at Rl 2: cell su = -1 reads rows 1 and 2 with weights 1/2, su = 0 row 2 alone, su = 1 rows 2 and 3
    layer = np.ones((1, 5, 5), np.float32)
    layer[0, 3, :] = np.nan
    st = NumpyScaledStack(1, 1).add_scaled(layer.reshape(1, -1), 2, 0.5)
    assert st.cnt.reshape(3, 3).tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0]]
    value, read, taps = resample(layer.reshape(1, -1), 2, np.zeros((1, 2), np.int32), 1, 0.5)
    assert read.all() and taps.reshape(3, 3).tolist() == [[4, 2, 4], [2, 1, 2], [4, 2, 4]]


def test_the_scaled_stack_over_six_time_baselines():
    """Six 8-bit pairs (160 x 160, +-100 DN of noise on image 1) whose motion is FB_OFFSET + s (2, -1) px, s = 1, 2, 0.5, 3, 1.5, 2; 60
    points, ocw 7, stack R 4; each layer searched at mimc3_stack_layer_radius around the layer shift.  Against their own truths the
    layers misplace 28, 22, 25, 27, 24 and 21 of the 60 points; the scaled stack of the six misplaces 1 (point 56, whose true peak lies
    on the border of its box: status -4); the unscaled stack of the same pairs (every layer at R 4 around the stack's shift)
    misplaces 58."""
    xy, shift = scaled_series_points()
    n = xy.shape[0]
    scaled, plain = NumpyScaledStack(n, SCALED_R, shift), NumpyStack(n, SCALED_R, shift)
    per_layer = []
    for s, i0, i1 in scaled_series_pairs():
        Rl = layer_radius(SCALED_R, s)
        rec, _, surf, _ = full_any(i0, i1, xy, FB_OFFSET, SCALED_OCW, Rl, 0, shift=layer_shift(shift, s))
        per_layer.append(int(misplaced(rec, layer_truth(s)).sum()))
        scaled.add_scaled(surf, Rl, s, 1.0, refused_of(rec))
        rec0, _, surf0, _ = full_any(i0, i1, xy, FB_OFFSET, SCALED_OCW, SCALED_R, 0, shift=shift)
        plain.add(surf0, refused_of(rec0))
    rec = scaled.finish()[0]
    stacked = int(misplaced(rec, SCALED_MOTION).sum())
    unscaled = int(misplaced(plain.finish()[0], SCALED_MOTION).sum())
    print(f"noise +-{SCALED_NOISE_DN} DN: misplaced per layer {per_layer}, scaled stack {stacked}, unscaled stack {unscaled}")
    assert min(per_layer) > 0, per_layer
    assert stacked < min(per_layer), (stacked, per_layer)
    assert unscaled > stacked, (unscaled, stacked)
    assert (per_layer, stacked, unscaled) == SCALED_COUNTS and rec[56, 2] == -4
