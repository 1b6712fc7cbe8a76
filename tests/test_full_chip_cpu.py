"""CPU: what the GPU tests of the exhaustive search at any chip size (tests/test_full_chip.py) rest on, without a device.

  * the oracle's two summation orders agree within 1 f32 ulp on the wide-range fixtures and bit for bit on the float_case fixtures at
    chip sizes up to 80: the GPU tests' conditions are ones the definition alone meets;
  * every fixture a GPU test uses holds at least three clean points, three dirty points and one fitted point;
  * the band rule in Python terms equals the library's query, stays inside the LDS budget, and has the band-boundary chip sizes the
    GPU tests derive from it; the multi-band fixtures hold the mixed points (a dirty point with a clean band; a point whose only null
    sits in the last row, or the last column, of its box);
  * chip_status_case has the statuses it is built for."""
import numpy as np
import pytest

import full_chip_common as fc
from conftest import assert_bits_equal
from full_any_common import full_any, surface_distance
from full_multi_common import STATUS_R

ALL_FIXTURES = sorted(set(fc.small_fixtures() + fc.radius_fixtures() + fc.band_fixtures() + fc.mode1_fixtures()))


@pytest.mark.parametrize("ocw", [10, 11, 20, 64, 80])
def test_oracle_orders_agree(ocw):
    radius = 7
    for kind in ("wide", "float"):
        c, f0, f1, shift = fc.chip_case(kind, ocw, radius, "zero")
        rec, _, a, _ = full_any(f0, f1, c.xyuvav, c.offset, ocw, radius, 0, shift=shift, order=0)
        b = full_any(f0, f1, c.xyuvav, c.offset, ocw, radius, 0, shift=shift, order=1)[2]
        share, worst = surface_distance(b, a, f"{kind} ocw {ocw}: the oracle's two orders")
        print(f"{kind} ocw {ocw}: {share:.6f} of the cells differ between the two orders, at most {worst} ulp")
        assert np.isfinite(a).any() and ((rec[:, 2] >= -1) | (rec[:, 2] == -4)).all()
        if kind == "float":
            assert_bits_equal(b, a, f"float_case ocw {ocw}: exact sums in both orders")
        else:
            assert worst <= 1


@pytest.mark.parametrize("kind,ocw,radius,enc,swap", ALL_FIXTURES)
def test_fixture_counts(kind, ocw, radius, enc, swap):
    c, i0, i1, shift = fc.chip_case(kind, ocw, radius, enc)
    sgn = -1 if swap else 1
    bands = fc.band_classes(i0, i1, c.xyuvav, sgn * c.offset, sgn * shift, ocw, radius, swap)
    clean, dirty, mixed = fc.class_counts(bands)
    rec = full_any(i0, i1, c.xyuvav, sgn * c.offset, ocw, radius, 0, shift=sgn * shift, swap=swap)[0]
    fitted = int((rec[:, 2] >= -1).sum())
    print(f"{kind} ocw {ocw} R {radius} {enc} swap {swap}: {clean} clean, {dirty} dirty ({mixed} mixed), {fitted} fitted of {c.n}")
    assert c.n <= 20 and clean >= 3 and dirty >= 3 and fitted >= 1
    if len(bands[0]) > 1:                                       # a multi-band chip: the mixed points of the placed nulls
        last_row, last_col = fc.only_null_in_last_box_line(i1, c.xyuvav, c.offset, shift, ocw, radius)
        assert mixed >= 1 and last_row and last_col
        assert any(b[-1] and not any(b[:-1]) for b in (bands[g] for g in last_row))         # the last band alone is dirty


def test_band_rule():
    from mimc3_amd import api
    assert api.full_chip_max_ocw() == fc.MAX_OCW
    for ocw in range(0, fc.MAX_OCW + 2):
        for radius in range(0, 17):
            assert api.full_chip_band_rows(ocw, radius) == fc.band_rows(ocw, radius), (ocw, radius)
    for ocw in range(1, fc.MAX_OCW + 1):
        for radius in range(1, 16):
            L = fc.layout(ocw, radius)
            assert 1 <= L["BR"] <= L["CW"]
            assert 2 * (L["lds"] + 1024) <= 160 * 1024           # two workgroups a compute unit, static slots included
            if L["BR"] < L["CW"]:                                # the largest band that fits: one more row would not
                assert L["lds"] <= fc.LDS_BUDGET < L["lds"] + 4 * (L["PB"] + L["CWP"])
    assert [fc.band_rows(o, 15) for o in (1, 41, 42, 64, 80)] == [3, 83, 77, 51, 39]
    cases = fc.band_shape_cases()
    assert set(cases) == set(fc.BAND_SHAPES)
    assert cases["one_band"] == (41, 15)
    for shape, (ocw, radius) in cases.items():
        assert fc.band_shape(2 * ocw + 1, fc.band_rows(ocw, radius)) == shape


@pytest.mark.parametrize("ocw", [10, 64])
def test_status_case(ocw):
    i0, i1, xy, shift = fc.chip_status_case(ocw)
    rec, cand, surf, nlm = full_any(i0, i1, xy, (0, 0), ocw, STATUS_R, 4, shift=shift)
    st = rec[:, 2]
    assert st[0] == -3 and np.isnan(surf[0]).all()
    assert st[1] == -2 and not np.isfinite(surf[1]).any()
    assert st[2] == -4 and (cand[:, 2, 2] >= -1).any()          # the interior local maxima are the candidates
    assert (st[3:6] != -3).all() and np.isfinite(surf[3:6]).any(axis=1).all()
    assert st[6] >= -1 and abs(rec[6, 0] - 5) < 0.5 and abs(rec[6, 1]) < 0.5     # (the record's offset includes the shift)
    bands = fc.band_classes(i0, i1, xy, (0, 0), shift, ocw, STATUS_R)
    assert all(any(b) for b in bands[3:6]) and not any(bands[2])  # the overhanging boxes meet the zero border
