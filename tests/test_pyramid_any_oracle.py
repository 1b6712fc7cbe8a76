"""CPU: the test-side definition of the coarse-to-fine search on any f32 pair (tests/pyramid_any_oracle.py) -- the float reduction on
hand-built blocks, its agreement with the integer reduction where the two must agree, the reach of three levels, and the share of
points at which the definition leaves the arg-max of a coarser level to the summation order (capped; the GPU test leaves those out)."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from pyramid_any_oracle import (ORACLE_CASES, ORACLE_LEVELS, ORACLE_R, UNDECIDED_CAP, big_float_case, hand_blocks, oracle_case, pyramid_any,
                                pyramid_search_any, reduce2_any, undecided_peaks, upsampled_pair)
from pyramid_dn_oracle import pyramid_dn
from pyramid_oracle import BIG


def test_hand_built_blocks():
    img, want = hand_blocks()
    lv = reduce2_any(img)
    assert lv.shape == (3, 14) and lv.dtype == np.float32           # 7 x 29: the odd row and column are dropped
    with np.errstate(over="ignore"):
        assert_bits_equal(lv[0], want.astype(np.float32), "hand-built blocks")
    assert lv[0, 4] == 0 and lv[0, 5] == 0 and not np.signbit(lv[0, 4:6]).any()     # n = 0 and the all-NaN block: +0
    assert np.isposinf(lv[0, 10:12]).all()
    assert lv[0, 13] == np.float32(4194304.75)                       # 2^22 + 0.75 is an f32; an f32 sum would have lost the 3
    assert np.isfinite(lv[1:]).all() and (lv[1:] > 0).all()
    for n in range(5):                                               # every n, one value: the mean is the value
        b = np.zeros((2, 2), np.float32)
        b.ravel()[:n] = np.float32(0.37)
        assert reduce2_any(b)[0, 0] == (np.float32(0.37) if n else 0)
    assert_bits_equal(reduce2_any(np.full((2, 2), np.nan, np.float32)), np.zeros((1, 1), np.float32), "all NaN")
    assert reduce2_any(np.ones((5, 7), np.float32)).shape == (2, 3)


@pytest.mark.parametrize("bits", [8, 12, 16])
def test_float_levels_of_an_upsampled_integer_pair_are_the_integer_levels(bits):
    i0, i1, _ = upsampled_pair(bits, 9100 + bits)
    for img in (i0, i1):
        assert ((img == 0).mean() > 0.002) and (img == np.rint(img)).all()
        f, d = pyramid_any(img, 3), pyramid_dn(img, 3)
        for lv in (1, 2):
            assert_bits_equal(f[lv], d[lv], f"{bits}-bit, level {lv}")
        assert (f[1] == 0).sum() < (img == 0).sum()                 # a punched pixel alone does not make a null


def test_three_levels_reach_the_large_displacement_as_floats():
    f0, f1, g = big_float_case()
    du, dv = BIG["motion"]
    ocw = BIG["ocw"]
    one, _, sh1, _ = pyramid_search_any(f0, f1, g, (0, 0), ocw, 15, 1)
    rec, _, sh, und = pyramid_search_any(f0, f1, g, (0, 0), ocw, 15, 3)
    assert not sh1.any()
    hit1 = (np.abs(one[:, 0] - du) < 0.05) & (np.abs(one[:, 1] - dv) < 0.05)
    assert hit1.mean() < 0.1
    ok = rec[:, 2] >= -1
    hit = ok & (np.abs(rec[:, 0] - du) < 0.05) & (np.abs(rec[:, 1] - dv) < 0.05)
    assert ok.sum() > 0 and hit.sum() >= 0.9 * ok.sum()
    assert und.mean() <= UNDECIDED_CAP


def test_undecided_peaks():
    one = np.float32(0.5)
    up = lambda x, k: np.float32(x).view(np.int32).__add__(k).view(np.float32)
    surf = np.array([[0.1, one, up(one, 3), np.nan],                # leads by 3 ulps: decided
                     [0.1, one, up(one, 2), np.nan],                # by 2: not
                     [one, one, 0.1, 0.2],                          # a tie: not
                     [np.nan, 0.3, np.nan, np.nan],                 # one finite cell: decided
                     [np.nan, np.nan, np.nan, np.nan]], np.float32)
    assert undecided_peaks(surf).tolist() == [False, True, True, False, False]


@pytest.mark.parametrize("kind,ocw", ORACLE_CASES)
def test_the_undecided_share_stays_within_the_cap(kind, ocw):
    """The condition of tests/test_pyramid_any.py::test_against_the_reference_order_oracle, on the oracle alone."""
    c, f0, f1, shift = oracle_case(kind, ocw)
    seen = 0
    for swap in (False, True):
        off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
        rec, _, sh, und = pyramid_search_any(f0, f1, c.xyuvav, off, ocw, ORACLE_R, ORACLE_LEVELS, shift=sh_in, swap=swap)
        print(f"{kind} ocw {ocw} swap {swap}: {int(und.sum())} of {c.n} points undecided")
        assert und.mean() <= UNDECIDED_CAP
        seen += int((rec[:, 2] >= -1).sum())
    assert seen > 0
