"""The advance list of the u8 matcher step, without a GPU: the rule of u8_classify (mx_climb_area, match_kernel.h) restated in numpy
(tests/u8_advance_common.py).  On BASELINE C2 the number of advance points is put on record next to the unchanged class counts, and on
every small fixture of tests/test_u8_advance.py both outcomes occur: window-null points on the list and window-null points off it."""
import numpy as np
import pytest

import u8_advance_common as ac
from mimc3_amd import synth
from test_u8_step_lists import C2_CLASSES

C2_ADVANCE = 17814          # of C2's 67,608 window-null points: the climb area (pivot rectangle grown by 2 cells, clipped) is null-free


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def test_axis_geometry_by_hand():
    """ocw 16, last pivot +14: dx2 32, 34 cells, reachable 1..32 (the tile holds them: origin 1); pivot cells 16..30, grown 14..32, their
    boxes reach pixel 64, clipped to the 64 written columns: 50 pixels from 14; last pivot -3: cells 5..2, grown and clipped to 1..7"""
    fits, t0, a0, a1, p0, n = (int(v) for v in ac.axis_geometry(np.array(14), 16))
    assert (fits, t0, a0, a1, p0, n) == (1, 1, 14, 32, 14, 50)
    fits, t0, a0, a1, p0, n = (int(v) for v in ac.axis_geometry(np.array(-3), 16))
    assert (fits, t0, a0, a1, p0, n) == (1, 1, 1, 7, 1, 39)
    assert not bool(ac.axis_geometry(np.array(30), 16)[0])      # a corridor wider than the tile


def test_c2_advance_points_on_record(api):
    c = synth.make_case("C2")
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, 16, *c.i0.shape)
    k = ac.classify(c.i0, c.i1, c.xyuvav, c.offset, off, uv, 16)
    chip, win = k["chip_n"] != 0, k["win_n"] != 0
    assert k["takes"].all()
    assert (int((~win & ~chip).sum()), int((win & ~chip).sum()), int((~win & chip).sum()), int((win & chip).sum())) == C2_CLASSES
    assert int(k["clean"].sum()) == C2_CLASSES[0] and int(k["wn"].sum()) == C2_CLASSES[1]
    assert int(k["advance"].sum()) == C2_ADVANCE
    assert not (k["advance"] & ~k["wn"]).any()


@pytest.mark.parametrize("ocw", (7, 16, 40))
def test_border_fixtures_decide_both_ways(api, ocw):
    """every side and every corner has a spot outside the area and inside the written window in one of the two flow directions; there the
    target point is on the list, and with the null just inside the area it is not"""
    seen = set()
    for flip in (False, True):
        for spot in ac.BORDER_SPOTS:
            case, in_window, g = ac.border_case(api, ocw, spot, flip)
            if not in_window:
                continue
            k = ac.classify(*case)
            assert k["wn"][g], (ocw, spot, flip)
            assert bool(k["advance"][g]) == spot.startswith("out_"), (ocw, spot, flip)
            seen.add(spot)
    assert seen == set(ac.BORDER_SPOTS), sorted(set(ac.BORDER_SPOTS) - seen)
    if ocw == 40:       # the area's rectangle is beyond one packed table query
        assert int(k["aw"][g]) * int(k["ah"][g]) > 8224


@pytest.mark.parametrize("ocw", (7, 16))
@pytest.mark.parametrize("name", ("t4", "blobs", "off_corridor"))
def test_mixed_fixtures_hold_both_outcomes(api, name, ocw):
    fn = dict(t4=ac.t4_case, blobs=ac.blobs_case, off_corridor=ac.off_corridor_case)[name]
    i0, i1, xy, offset, off, uv, _ = fn(api, ocw)
    k = ac.classify(i0, i1, xy, offset, off, uv, ocw)
    assert k["advance"].any() and (k["wn"] & ~k["advance"]).any() and k["clean"].any(), (name, ocw)
    if name == "t4":    # some advance point's area ends at the last reachable cell on the far side: its boxes end at the written area's edge
        far = k["advance"] & ((k["ax"] + k["aw"] == k["wu"] + 2 * k["dx2"]) | (k["ay"] + k["ah"] == k["wv"] + 2 * k["dy2"]))
        assert far.any()
