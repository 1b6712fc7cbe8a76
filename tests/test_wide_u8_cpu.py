"""CPU: the facts the GPU tests of mimc3_match_ncc_wide_class (tests/test_wide_u8.py) rely on -- the library's radius and layout
queries against a Python restatement of the layout, the make-up of every placed-null fixture (clean and dirty workgroups, one point of
every status), and the oracle's own facts about the seam pairs: where the tied maxima lie.  No device."""
import numpy as np
import pytest

import wide_u8_common as wu
from full_any_common import full_any
from wide_common import FAR_R, FAR_TRUE, far_case, tail_decisions_py


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def test_max_radius(api):
    for ocw in range(1, 81):
        assert api.wide_class_max_radius(ocw) == 47
    for ocw in (-1, 0, 81, 1000):
        assert api.wide_class_max_radius(ocw) == 0


def test_layout_query_is_the_layout(api):
    worst = 0
    for ocw in range(1, 81):
        for R in range(16, 48):
            got = api.wide_class_layout(ocw, R)
            assert got == wu.layout(ocw, R), (ocw, R)
            assert got[3] <= 160 * 1024 and got[2] == 128 and got[1] == (2 * R + 1 + 31) // 32
            worst = max(worst, got[3])
    assert worst == api.wide_class_layout(80, 47)[3]
    for ocw, R in ((0, 16), (81, 16), (16, 15), (16, 48), (16, 0)):
        assert api.wide_class_layout(ocw, R) is None and wu.layout(ocw, R) is None
    assert [api.wide_class_layout(o, 16)[0] for o in (24, 25, 56, 57)] == [1, 2, 2, 3]


def test_case_table():
    assert all((o, r) in wu.CASES for o in (7, 16) for r in wu.RADII)
    assert all((o, r) in wu.CASES for o in wu.OCWS for r in (16, 47)) and (80, 32) in wu.CASES
    assert all(o in wu.SIX for o, r in wu.SIX_CASES) and all(o not in wu.SIX for o, r in wu.OUTSIDE_CASES)


@pytest.mark.parametrize("fx", wu.all_fixtures(), ids=lambda t: "ocw%d-R%d%s%s%s" % (t[0], t[1], "-swap" if t[2] else "", "" if t[3] else "-noshift", "-sat" if t[4] else ""))
def test_fixture_holds_every_kind_of_point(fx):
    f = wu.fixture(*fx)
    clean, dirty, r3c, r3b = wu.kinds(f)
    assert clean.sum() >= 3 and dirty.sum() >= 3, (clean.sum(), dirty.sum())
    assert list(np.flatnonzero(r3c)) == [wu.G3CHIP] and list(np.flatnonzero(r3b)) == [wu.G3BOX]
    assert clean[wu.G4] and clean[wu.CLEAN] and clean[wu.OUTSIDE] and dirty[wu.ONE_TILE] and dirty[:6].all()
    # the oracle's statuses of the doctored points: -4 on the border of the range, in the last tile column; -3 twice
    pts = [wu.G4, wu.G3CHIP, wu.G3BOX]
    rec, _, surf, _ = full_any(f["i0"], f["i1"], f["xy"][pts], f["off"], f["ocw"], f["R"], 0,
                               shift=None if f["shift"] is None else f["shift"][pts], swap=f["swap"])
    assert rec[0, 2] == -4 and rec[1, 2] == -3 and rec[2, 2] == -3 and np.isnan(surf[1:]).all()
    S = 2 * f["R"] + 1
    status, k, _ = tail_decisions_py(surf[0].reshape(S, S), 0)
    assert status == -4 and k // S == S - 1 and k % S == f["R"] + 3
    assert (S - 1) // 32 == (S + 31) // 32 - 1                 # (the last tile column)


@pytest.mark.parametrize("period", wu.SEAM_PERIODS)
def test_seam_pairs_tie_across_tiles(period):
    """the oracle's own facts: the maxima are exactly tied at 1, lie on both sides of the tile seams, and the first in k wins"""
    p0, p1, xy = wu.seam_pair(*period, plateau=False)
    rec, cand, surf, nlm = full_any(p0, p1, xy[:2], (0, 0), wu.SEAM_OCW, wu.SEAM_R, 8)
    S = 2 * wu.SEAM_R + 1
    xs, ys = wu.maxima_cells(period[0]), wu.maxima_cells(period[1])
    if period == (16, 16):
        assert 31 in xs and 63 in xs and 31 in ys and 63 in ys
    else:
        assert 32 in xs and 64 in ys
    assert len({x // 32 for x in xs}) == 3 and len({y // 32 for y in ys}) == 3     # tied maxima in every tile
    for g in range(2):
        v = surf[g].reshape(S, S)
        top = v.max()
        assert all(v[x, y] == top for x in xs for y in ys)
        status, k, ranked = tail_decisions_py(v, 8)
        assert status is None and k == xs[0] * S + ys[0] and nlm[g] >= len(xs) * len(ys)
        assert list(ranked) == sorted(x * S + y for x in xs for y in ys)[:8]      # ties rank in k order: across tiles


@pytest.mark.parametrize("R,y", wu.SEAM_PLATEAUS)
def test_seam_plateau(R, y):
    """a chip of one whole period (15 px at ocw 7): the top is flat over the cells y | y + 1, on both sides of a tile seam"""
    p0, p1, xy = wu.seam_pair(*wu.PLATEAU_PERIOD, plateau=True)
    rec, cand, surf, nlm = full_any(p0, p1, xy[:1], (0, 0), wu.SEAM_OCW, R, 8)
    S = 2 * R + 1
    v = surf[0].reshape(S, S)
    assert (y + 1) % 32 == 0 and v[R, y] == v[R, y + 1] and v[R, y] == v.max()
    _, _, ranked = tail_decisions_py(v, 8)
    assert len(ranked) == 8 and all((k % S - R) % wu.PLATEAU_PERIOD[1] == 0 for k in ranked)      # a plateau yields its lowest k alone
    assert any(k % S == y for k in ranked)


def test_far_pair_is_within_reach_of_both_chip_sizes():
    c = far_case()
    for ocw in (16, 10):
        rec, _, _, _ = full_any(c.i0, c.i1, c.xyuvav, (0, 0), ocw, FAR_R, 0)
        assert np.isfinite(rec[:, 0]).all()
        assert np.hypot(rec[:, 0] - FAR_TRUE[0], rec[:, 1] - FAR_TRUE[1]).max() < 0.5
