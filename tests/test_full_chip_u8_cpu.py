"""CPU: what the GPU tests of the exhaustive search on 8-bit pairs at any chip size on the matrix cores (tests/test_full_chip_u8.py) rest
on, without a device.

  * the new symbols are declared in the header and exported by the library; the layout in Python terms is the library's, fits a compute
    unit's LDS at every ocw (two workgroups at the largest chip), and has the boundary chip sizes the GPU tests derive from it;
  * every fixture a GPU test uses, counted in numpy and run through the float-pixel oracle: at least 3 clean points, 2 with nulls in the
    box only, 2 in the chip only, 2 on both sides, 1 fitted point;
  * the integer bounds the kernel states, in integer arithmetic;
  * on the saturated fixtures ONE packed table query of a chip is wrong at ocw 45 and right at ocw 44, and the sub-box split is right at
    both: the GPU cases at 44 | 45 can tell a kernel that queries the chip whole."""
import os
import re

import numpy as np
import pytest

import full_chip_u8_common as fu
import value_limit_common as vl
from conftest import ROOT
from full_any_common import full_any

SYMBOLS = ("mimc3_match_ncc_full_chip_class", "mimc3_match_ncc_full_chip_class_dev", "mimc3_full_chip_class_layout")


def test_symbols_are_declared_and_exported():
    from mimc3_amd import api
    header = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/mimc3_hip.h"
        assert getattr(api._lib, name) is not None
    assert " 12 = " in header and "u8_mfma_chip" in open(os.path.join(ROOT, "mimc3_amd", "api.py")).read()
    assert hasattr(api.Context, "match_ncc_full_chip_class") and hasattr(api.Context, "match_ncc_full_chip_class_dev")


def test_layout_is_the_librarys_and_fits():
    from mimc3_amd import api
    assert api.full_chip_max_ocw() == fu.MAX_OCW
    for ocw in range(0, fu.MAX_OCW + 2):
        assert api.full_chip_class_layout(ocw) == fu.layout_tuple(ocw), ocw
    for ocw in range(1, fu.MAX_OCW + 1):
        L = fu.layout(ocw)
        assert 1 <= L["KCW"] <= 3 and L["KCW"] == -(-(L["CW"] + 15) // 64)          # the issue's formula
        assert L["NTR"] <= 12 and L["KCV"] <= 3 and L["lds"] <= 160 * 1024
    assert 2 * fu.layout(fu.MAX_OCW)["lds"] <= 160 * 1024
    b = fu.boundaries()
    assert b["KCW"] == [(24, 25), (56, 57)]
    assert b == fu.boundaries(api.full_chip_class_layout)
    assert all(len(v) >= 2 for v in b.values())
    sizes = [o for o, _ in fu.size_cases()]
    assert {1, 2, 3, 10, 11, 14, 24, 25, 56, 57, 60, 80} <= set(sizes)
    assert {(2 * o + 1) % 4 for o in (1, 2, 3)} == {1, 3}


def test_integer_bounds():
    cw, top = 2 * fu.MAX_OCW + 1, 255
    assert cw * cw * top * top == 1685513025 < 2 ** 31                  # the largest true sum
    assert cw * cw * 128 * 128 < 2 ** 29                                # offset form, and a correlation with a null plane (-128 per null)
    assert cw * top * top < 2 ** 24 and cw * top < 2 ** 16 and cw < 256  # row-box sums: three, two, one byte plane
    assert 0.98 * 2 ** 31 < cw * cw * 128 * 128 + 128 * 2 * cw * cw * top < 2 ** 31      # sum a'b' + 128 (sx + sy): why sum ab is put together in f64
    sh = vl.sat_shifts()
    sq, nl = sh["kSatSqShift8"], sh["kSatNullShift8"]
    assert 64 * 64 * top < 2 ** sq and 64 * 64 * top * top < 2 ** (nl - sq) and 64 * 64 < 2 ** (64 - nl)     # a sub-box fits every field
    assert 89 * 89 <= vl.PACKED_QUERY_PIXELS < 91 * 91                  # ocw 44 | 45
    assert 91 * 91 * top >= 2 ** sq                                     # ... where a saturated chip's sum carries


@pytest.mark.parametrize("ocw,radius,swap,with_shift,saturated", fu.all_fixtures())
def test_fixture_counts(ocw, radius, swap, with_shift, saturated):
    c, i0, i1, shift = fu.u8_case(ocw, radius, "placed", swap, with_shift, saturated)
    assert c.n <= 20 and i0.max() <= 255 and np.array_equal(i0, np.rint(i0)) and np.array_equal(i1, np.rint(i1))
    nc, nb = fu.null_counts(c, i0, i1, shift, ocw, radius, swap)
    clean, box_only, chip_only, both = (nc == 0) & (nb == 0), (nc == 0) & (nb > 0), (nc > 0) & (nb == 0), (nc > 0) & (nb > 0)
    assert list(np.flatnonzero(box_only)) == list(fu.BOX_ONLY) and list(np.flatnonzero(chip_only)) == list(fu.CHIP_ONLY)
    assert list(np.flatnonzero(both)) == list(fu.BOTH) and clean.sum() >= 3
    assert (nc <= 1).all() and (nb <= 1).all()                          # single nulls
    sgn = -1 if swap else 1
    rec = full_any(i0, i1, c.xyuvav, sgn * c.offset, ocw, radius, 0, shift=None if shift is None else sgn * shift, swap=swap)[0]
    fitted = rec[:, 2] >= -1
    print(f"ocw {ocw} R {radius} swap {swap} shift {with_shift} saturated {saturated}: {int(fitted.sum())} fitted of {c.n}")
    assert fitted.sum() >= 1 and (rec[:, 2] != -3).all()


def test_the_other_null_patterns():
    c, i0, i1, shift = fu.u8_case(10, 7, "none")
    nc, nb = fu.null_counts(c, i0, i1, shift, 10, 7, False)
    assert not nc.any() and not nb.any()
    c, i0, i1, shift = fu.u8_case(10, 7, "all")
    nc, nb = fu.null_counts(c, i0, i1, shift, 10, 7, False)
    assert (nb > 0).all() and (nc > 0).sum() >= 2 and (nc == 0).sum() >= 2


@pytest.mark.parametrize("spread", [1, 3])
def test_one_packed_query_fails_at_45_and_not_at_44(spread):
    sh = vl.sat_shifts()
    sq, nl = sh["kSatSqShift8"], sh["kSatNullShift8"]
    for ocw, whole_is_right in ((44, True), (45, False)):
        c, i0, i1, shift = fu.u8_case(ocw, 15, "placed", saturated=spread)
        q = i0.astype(np.int64)
        cw = 2 * ocw + 1
        S = vl.table(vl.pack_u8(q, sq, nl))
        u, v = vl.grid_uv(c.xyuvav)
        y, x = v - ocw, u - ocw                                         # the chips' top-left pixels
        true = [vl.box_sums(vl.table(w), cw, cw)[y, x] for w in (q, q * q, (q == 0).astype(np.int64))]
        whole = [f[y, x].astype(np.int64) for f in vl.unpack_u8(vl.box_sums(S, cw, cw), sq, nl)]
        split = [np.zeros(c.n, np.int64) for _ in range(3)]
        for j in range(0, cw, 64):
            for i in range(0, cw, 64):
                w0, h0 = min(cw - i, 64), min(cw - j, 64)
                for k, f in enumerate(vl.unpack_u8(vl.box_sums(S, w0, h0), sq, nl)):
                    split[k] += f[y + j, x + i].astype(np.int64)
        for k in range(3):
            assert np.array_equal(split[k], true[k].astype(np.int64)), (ocw, k)
        right = all(np.array_equal(whole[k], true[k].astype(np.int64)) for k in range(3))
        assert right == whole_is_right, f"ocw {ocw}: one packed query is {'right' if right else 'wrong'}"
