"""CPU: the test-side definition of the coarse-to-fine search on every pair class (tests/pyramid_dn_oracle.py) against the oracles it
restates -- the 8-bit pyramid definition (tests/pyramid_oracle.py), the integer exhaustive search on the integer levels of a 12-bit
pair, its own scale invariance -- and the parity fixtures' power to tell rounded from exact products on every level."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_dn_common import differing_fraction
from full_search_common import full_search
from pyramid_dn_oracle import as_class, case, pyramid_dn, pyramid_search_dn, reduce2_dn
from pyramid_oracle import _inside, big_case, pyramid, pyramid_search

R = 6


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_equals_the_8bit_definition(levels):
    c = case(16, 0.03, 8101)
    shift = np.rint(np.random.default_rng(1).normal(0, 2, (c.n, 2))).astype(np.int32)
    for swap in (False, True):
        off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
        want, want_sh = pyramid_search(c.i0, c.i1, c.xyuvav, off, 16, R, levels, shift=sh_in, swap=swap)
        rec, cand, sh = pyramid_search_dn(c.i0, c.i1, c.xyuvav, off, 16, R, levels, shift=sh_in, swap=swap)
        assert cand is None
        np.testing.assert_array_equal(sh, want_sh)
        assert_bits_equal(rec, want, f"L {levels} swap {swap}")
    for a, b in zip(pyramid(c.i0, levels), pyramid_dn(c.i0, levels)):
        np.testing.assert_array_equal(a, b)


def test_equals_the_8bit_definition_on_the_large_displacement():
    i0, i1, g = big_case()
    want, want_sh = pyramid_search(i0, i1, g, (0, 0), 32, 15, 3)
    rec, _, sh = pyramid_search_dn(i0, i1, g, (0, 0), 32, 15, 3)
    np.testing.assert_array_equal(sh, want_sh)
    assert_bits_equal(rec, want, "big_case")


def test_level_peaks_on_a_12bit_pair_are_the_integer_search():
    """Shift 0: the levels are integers below 4096, where every product is exact -- the integer oracle's arg-max cells, level by level."""
    c = case(16, 0.03, 8102)
    i0, i1 = as_class("u16", c)
    _, _, sh, peaks = pyramid_search_dn(i0, i1, c.xyuvav, c.offset, 16, R, 3, with_peaks=True)
    p0, p1 = pyramid_dn(i0, 3), pyramid_dn(i1, 3)
    assert all(lv.max() < 4096 and (lv == np.rint(lv)).all() for lv in p0 + p1)
    uv0 = c.xyuvav[:, 2:4].astype(np.int64)
    d = (np.asarray(c.offset, np.int64).reshape(1, 2) + np.zeros((c.n, 2), np.int64) + 2) >> 2
    S = 2 * R + 1
    seen = 0
    for k, lv in enumerate((2, 1)):
        H, W = p0[lv].shape
        ok = _inside(uv0 >> lv, d, 16, R, H, W)
        xy = np.zeros((int(ok.sum()), 6))
        xy[:, 2:4] = (uv0 >> lv)[ok]
        pk = np.full(c.n, -1, np.int64)
        pk[ok] = full_search(p0[lv], p1[lv], xy, (0, 0), 16, R, shift=d[ok].astype(np.int32), with_peak=True)[1]
        np.testing.assert_array_equal(peaks[k], pk)
        seen += int((pk >= 0).sum())
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - R, pk % S - R], axis=1), 0)
        d = 2 * (d + s)
    assert seen > 0
    np.testing.assert_array_equal(sh, (d - np.asarray(c.offset, np.int64)).astype(np.int32))


@pytest.mark.parametrize("cls", ["u16", "f32"])
def test_a_pair_divided_by_8_gives_the_same_result(cls):
    c = case(16, 0.03, 8103)
    i0, i1 = as_class(cls, c)
    a = pyramid_search_dn(i0, i1, c.xyuvav, c.offset, 16, R, 3, npeaks=4)
    b = pyramid_search_dn(i0 / np.float32(8), i1 / np.float32(8), c.xyuvav, c.offset, 16, R, 3, npeaks=4)
    np.testing.assert_array_equal(a[2], b[2])
    assert_bits_equal(a[0], b[0], "record")
    assert_bits_equal(a[1], b[1], "candidates")
    assert (a[0][:, 2] >= -1).any()
    np.testing.assert_array_equal(reduce2_dn(i0 / np.float32(8), 3) * np.float32(8), reduce2_dn(i0, 0))


def test_the_reduction_rounds_ties_up_and_skips_nulls():
    img = np.array([[5, 6, 0, 0, 7, 0, 1, 2],
                    [0, 0, 0, 0, 2, 2, 2, 1]], np.float32)
    np.testing.assert_array_equal(reduce2_dn(img, 0), [[6, 0, 4, 2]])           # 11/2 -> 6; none; (11 + 1) // 3; (6 + 2) // 4
    np.testing.assert_array_equal(reduce2_dn(img / np.float32(8), 3), np.array([[6, 0, 4, 2]], np.float32) / 8)
    top = np.array([[2 ** 20 - 1, 2 ** 20 - 1], [2 ** 20 - 1, 2 ** 20 - 1]], np.float32)
    np.testing.assert_array_equal(reduce2_dn(top, 0), [[2 ** 20 - 1]])
    np.testing.assert_array_equal(reduce2_dn(np.ones((5, 7), np.float32), 0), np.ones((2, 3), np.float32))


@pytest.mark.parametrize("ocw", [7, 16])
def test_16bit_fixtures_tell_rounded_from_exact_products_on_every_level(ocw):
    """A kernel with exact products must fail at every level: at least a quarter of the finite cells differ on each."""
    c = case(ocw, 0.03, 8200 + ocw)
    i0, i1 = as_class("f32", c)
    p0, p1 = pyramid_dn(i0, 3), pyramid_dn(i1, 3)
    uv0 = c.xyuvav[:, 2:4].astype(np.int64)
    for lv in range(3):
        H, W = p0[lv].shape
        d = np.zeros((c.n, 2), np.int64)
        ok = _inside(uv0 >> lv, d, ocw, R, H, W)
        assert ok.any()
        xy = np.zeros((int(ok.sum()), 6))
        xy[:, 2:4] = (uv0 >> lv)[ok]
        assert differing_fraction(p0[lv], p1[lv], xy, (0, 0), ocw, R) >= 0.25, f"level {lv}"
