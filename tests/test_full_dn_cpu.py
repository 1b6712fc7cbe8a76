"""CPU: the interface of the exhaustive search on integral-f32 pairs (mimc3_match_ncc_full_dn), and its test-side oracle
(tests/full_dn_oracle.c) against the two integer oracles, against the Python restatement of the reference's cell, and against its own
exact-product form on every 16-bit fixture the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_dn_common import (differing_fraction, dn16_case, full_dn, periodic_pair16, status_case16, c2_dn16, c2_sample)
from full_multi_common import STATUS_R, full_multi, parity_case
from full_planes_common import PLANES_OCW, PLANES_R, dn12_case, null_sides, status_case12, surface_f32
from full_search_common import full_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mimc3_match_ncc_full_dn", "mimc3_match_ncc_full_dn_dev")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared in mimc3_hip.h"
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"
    from mimc3_amd import api
    assert callable(getattr(api.Context, "match_ncc_full_dn", None)) and callable(getattr(api.Context, "match_ncc_full_dn_dev", None))


def _same_as_the_integer_oracles(i0, i1, xy, off, ocw, radius, shift, swap, what):
    want_rec = full_search(i0, i1, xy, off, ocw, radius, shift=shift, swap=swap)
    want_out, want = full_multi(i0, i1, xy, off, ocw, radius, 8, shift=shift, swap=swap)
    rec, none = full_dn(i0, i1, xy, off, ocw, radius, 0, shift=shift, swap=swap)
    assert none is None
    assert_bits_equal(rec, want_rec, what + ": record vs full_search")
    out, cand = full_dn(i0, i1, xy, off, ocw, radius, 8, shift=shift, swap=swap)
    assert_bits_equal(out, want_out, what + ": record vs full_multi")
    assert_bits_equal(cand, want, what + ": candidates vs full_multi")
    out4, cand4 = full_dn(i0, i1, xy, off, ocw, radius, 4, shift=shift, swap=swap)
    assert_bits_equal(out4, rec, what + ": record at npeaks 4")
    assert_bits_equal(cand4, want[:4], what + ": candidates, npeaks 4")


@pytest.mark.parametrize("ocw,null_frac,radius", [(7, 0.03, 7), (16, 0.0, 15), (16, 0.03, 7), (30, 0.03, 1)])
def test_oracle_equals_the_integer_oracles_on_8_and_12_bit(ocw, null_frac, radius):
    """Where every product is exact the rounded-product cell is the integer cell: records and candidates bit for bit."""
    c, shift = parity_case(ocw, null_frac, radius, dimx=5, dimy=4)
    for swap in (False, True):
        sgn = -1 if swap else 1
        _same_as_the_integer_oracles(c.i0, c.i1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap, f"8-bit swap {swap}")
    c, i0, i1, shift = dn12_case(ocw, null_frac, radius)
    _same_as_the_integer_oracles(i0, i1, c.xyuvav, c.offset, ocw, radius, shift, False, "12-bit")
    _same_as_the_integer_oracles(i0, i1, c.xyuvav, c.offset, ocw, radius, None, False, "12-bit, no shift")


def test_oracle_equals_the_integer_oracles_on_the_status_fixture():
    i0, i1, xy = status_case12()
    for radius in (STATUS_R, 1):
        _same_as_the_integer_oracles(i0, i1, xy, (0, 0), 7, radius, None, False, f"statuses R {radius}")


def test_surface_is_the_reference_cell_on_16_bit():
    """The oracle's surface against full_planes_common.ncc_cell_f32 (the reference's cell restated in numpy scalars) cell for cell, at
    points without nulls, with nulls in the chip alone, in the box alone and in both; on 16-bit DN and on DN / 8 against DN."""
    i0, i1, xy = status_case16()
    radius = 2
    sides = null_sides(i0, i1, xy, 7, radius)
    H, W = i0.shape
    pts = [g for g in range(xy.shape[0])
           if min(xy[g, 2], xy[g, 3]) >= 7 + radius and xy[g, 2] + 7 + radius < W and xy[g, 3] + 7 + radius < H and g != 0]
    kinds = {(c > 0, b > 0) for g, (c, b) in enumerate(sides) if g in pts}
    assert {(True, False), (True, True)} <= kinds, kinds
    extra = np.zeros((2, 6))
    extra[:, 2:4] = [[100, 30], [52, 92]]               # no null at all; a null in the box alone
    xy2 = np.concatenate([xy[pts], extra])
    sides2 = null_sides(i0, i1, xy2, 7, radius)
    assert any(c == 0 and b == 0 for c, b in sides2) and any(c == 0 and b > 0 for c, b in sides2), sides2
    for f0, f1, what in ((i0, i1, "DN"), (i0 / np.float32(8), i1, "DN / 8 against DN")):
        surf = full_dn(f0, f1, xy2, (0, 0), 7, radius, 0, with_surface=True)[2]
        for g in range(xy2.shape[0]):
            want = surface_f32(f0, f1, int(xy2[g, 2]), int(xy2[g, 3]), 7, radius)
            assert_bits_equal(surf[g], want, f"{what}: surface of point {g}")
    # and the scale is invisible in the record, as the kernel's argument for working on the integers needs it
    a = full_dn(i0, i1, xy2, (0, 0), 7, radius, 4)
    b = full_dn(i0 / np.float32(8), i1 / np.float32(8), xy2, (0, 0), 7, radius, 4)
    assert_bits_equal(a[0], b[0], "record, DN vs DN / 8")
    assert_bits_equal(a[1], b[1], "candidates, DN vs DN / 8")


def test_status_case16_holds_every_class():
    i0, i1, xy = status_case16()
    assert i0.max() <= 65535 and i0.max() > 4095
    out, cand, nlm = full_dn(i0, i1, xy, (0, 0), 7, STATUS_R, 4, with_counts=True)
    st = out[:, 2]
    assert (st == -2).any() and (st == -3).any() and (st == -4).any()
    sides = null_sides(i0, i1, xy, 7, STATUS_R)
    assert any(c > 0 and b == 0 for c, b in sides) and any(c == 0 and b > 0 for c, b in sides) and any(c > 0 and b > 0 for c, b in sides)
    assert any(c == 0 and b == 0 for c, b in sides)
    assert ((nlm < 4) & (st != -3)).any()


# ---- the fixture condition: a kernel that multiplies exactly must not pass.  On every 16-bit fixture of tests/test_full_dn.py at least a
#      quarter of the finite cells differ in their f32 bits between the reference's rounded products and exact ones ----
@pytest.mark.parametrize("radius", PLANES_R)
@pytest.mark.parametrize("null_frac", [0.0, 0.03])
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_fixture_tells_rounded_from_exact_products(ocw, null_frac, radius):
    c, i0, i1, shift = dn16_case(ocw, null_frac, radius)
    frac = differing_fraction(i0, i1, c.xyuvav, c.offset, ocw, radius, shift=shift)
    print(f"ocw {ocw} nulls {null_frac} R {radius}: {frac:.3f} of the cells differ")
    assert frac >= 0.25, frac


def test_other_fixtures_tell_rounded_from_exact_products():
    i0, i1, xy = status_case16()
    for radius in (STATUS_R, 1):
        assert differing_fraction(i0, i1, xy, (0, 0), 7, radius) >= 0.25
    p0, p1, pxy = periodic_pair16()
    assert differing_fraction(p0, p1, pxy, (0, 0), 15, 15) >= 0.25
    from mimc3_amd import api
    c, i0, i1 = c2_dn16()
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    sel = c2_sample(c.n)[::40]
    assert differing_fraction(i0, i1, c.xyuvav[sel], c.offset, 16, 15, shift=shift[sel]) >= 0.25
    # and the pair the old refusal test uses does NOT: multiples of 256 have exact products
    c8, sh8 = parity_case(16, 0.03, 7, dimx=5, dimy=4)
    assert differing_fraction(c8.i0 * 256, c8.i1 * 256, c8.xyuvav, c8.offset, 16, 7, shift=sh8) == 0.0
