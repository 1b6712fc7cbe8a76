"""CPU: the facts the GPU tests of mimc3_match_ncc_wide_planes (tests/test_wide_u16.py) rely on -- the library's radius and layout
queries against a Python restatement of the layout, the make-up of every placed-null 12-bit fixture (clean and dirty workgroups, one
point of every status, both 6-bit planes alive in every chip), the integer bounds of the two-plane arithmetic on a saturated chip of 161
pixels, and the oracle's own facts about the 12-bit seam pairs.  No device."""
import ctypes as C

import numpy as np
import pytest

import wide_u16_common as wp
from full_any_common import full_any
from full_chip_u16_common import spread12
from wide_common import FAR_R, FAR_TRUE, far_case, tail_decisions_py


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def test_abi_exports_the_four_symbols(api):
    for name in ("mimc3_match_ncc_wide_planes", "mimc3_match_ncc_wide_planes_dev", "mimc3_wide_planes_max_radius", "mimc3_wide_planes_layout"):
        assert C.cast(getattr(api._lib, name), C.c_void_p).value, name
    assert hasattr(api.Context, "match_ncc_wide_planes_dev") and callable(api.wide_planes_layout)


def test_max_radius(api):
    got = [api.wide_planes_max_radius(o) for o in range(1, 81)]
    assert got == [wp.max_radius(o) for o in range(1, 81)]
    assert all(r == 47 for r in got[:68]) and got[68:72] == [46, 45, 44, 43] and got[72:] == list(range(34, 26, -1))
    assert all(a >= b for a, b in zip(got[67:], got[68:]))                      # non-increasing from ocw 68 on
    assert all(16 <= r <= api.wide_class_max_radius(o + 1) for o, r in enumerate(got))
    for ocw in (-1, 0, 81, 1000):
        assert api.wide_planes_max_radius(ocw) == 0 and wp.max_radius(ocw) == 0


def test_layout_query_is_the_layout(api):
    worst = 0
    for ocw in range(1, 81):
        lim = api.wide_planes_max_radius(ocw)
        for R in range(16, 48):
            got = api.wide_planes_layout(ocw, R)
            assert got == wp.layout(ocw, R), (ocw, R)
            assert (got is None) == (R > lim)
            if got:
                assert got[3] <= 160 * 1024 and got[2] == 128 and got[1] == (2 * R + 1 + 31) // 32
                worst = max(worst, got[3])
        if lim < 47:                                                            # the limit is the LAST radius that fits
            assert wp.lds_bytes(ocw, lim + 1)[1] > 160 * 1024
    assert worst == api.wide_planes_layout(80, 27)[3] == 163680
    for ocw, R in ((0, 16), (81, 16), (16, 15), (16, 48), (16, 0), (80, 28), (69, 47)):
        assert api.wide_planes_layout(ocw, R) is None and wp.layout(ocw, R) is None
    assert [api.wide_planes_layout(o, 16)[0] for o in (24, 25, 56, 57)] == [1, 2, 2, 3]


def test_case_table():
    assert wp.STEPS == [69, 73] and wp.STEP_OCWS == [68, 69, 72, 73]
    assert all((o, r) in wp.CASES for o in (7, 16) for r in (16, 23, 31, 32, 47))
    assert all((o, r) in wp.CASES for o in (1, 24, 25, 44, 45, 56, 57) for r in (16, 47))
    assert all(c in wp.CASES for c in ((68, 47), (69, 46), (72, 43), (73, 34), (80, 16), (80, 27)))
    assert all(o in wp.SIX for o, r in wp.SIX_CASES) and all(o not in wp.SIX for o, r in wp.OUTSIDE_CASES)
    assert all(r <= wp.max_radius(o) for o, r in wp.CASES + wp.SIX_CASES + list(wp.SATURATED))


@pytest.mark.parametrize("fx", wp.all_fixtures(), ids=lambda t: "ocw%d-R%d-%s%s%s" % (t[0], t[1], t[2], "-swap" if t[3] else "", "" if t[4] else "-noshift"))
def test_fixture_holds_every_kind_of_point(fx):
    f = wp.fixture(*fx)
    ocw, R = f["ocw"], f["R"]
    clean, dirty, r3c, r3b = wp.kinds(f)
    assert clean.sum() >= 3 and dirty.sum() >= 3, (clean.sum(), dirty.sum())
    assert list(np.flatnonzero(r3c)) == [wp.G3CHIP] and list(np.flatnonzero(r3b)) == [wp.G3BOX]
    assert clean[wp.G4] and clean[wp.CLEAN] and clean[wp.OUTSIDE] and dirty[wp.ONE_TILE] and dirty[:6].all()
    # the oracle's statuses of the doctored points: -4 on the border of the range, in the last tile column; -3 twice
    pts = [wp.G4, wp.G3CHIP, wp.G3BOX]
    rec, _, surf, _ = full_any(f["i0"], f["i1"], f["xy"][pts], f["off"], ocw, R, 0,
                               shift=None if f["shift"] is None else f["shift"][pts], swap=f["swap"])
    assert rec[0, 2] == -4 and rec[1, 2] == -3 and rec[2, 2] == -3 and np.isnan(surf[1:]).all()
    S = 2 * R + 1
    status, k, _ = tail_decisions_py(surf[0].reshape(S, S), 0)
    assert status == -4 and k // S == S - 1 and k % S == R + 3
    assert (S - 1) // 32 == (S + 31) // 32 - 1                 # (the last tile column)
    # the two 6-bit planes of q = 64 h + l in every chip (but the one nulled for the -3): the low plane never constant; the high plane
    # never constant on a spread pair -- a pair pressed against 4095 holds h = 63 on every pixel that is not a null, which is its point
    q0, q1 = wp.planes(f)
    chip_img = q1 if f["swap"] else q0
    u, v = f["xy"][:, 2].astype(int), f["xy"][:, 3].astype(int)
    for g in range(f["xy"].shape[0]):
        if g == wp.G3CHIP:
            continue
        q = chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
        assert (q & 63).min() != (q & 63).max(), g
        if f["kind"] in ("sat3", "sat63"):
            assert (q[q > 0] >> 6).min() == 63
        else:
            assert (q >> 6).min() != (q >> 6).max(), g


@pytest.mark.parametrize("spread", [3, 63])
def test_two_plane_arithmetic_on_a_saturated_chip_of_161(spread):
    """sum ab = 4096 HH + 64 (SS - HH - LL) + LL with SS = sum (h + l)(h' + l'): exact, below 2^39, every correlation inside an i32"""
    rng = np.random.default_rng(161 + spread)
    a = rng.integers(4095 - spread, 4096, (161, 161), dtype=np.int64)
    b = rng.integers(4095 - spread, 4096, (161, 161), dtype=np.int64)
    a[0, 0] = b[3, 5] = 4095
    ah, al, bh, bl = a >> 6, a & 63, b >> 6, b & 63
    assert max(ah.max(), al.max(), bh.max(), bl.max()) <= 63 and (ah + al).max() <= 126
    HH, LL, SS = int((ah * bh).sum()), int((al * bl).sum()), int(((ah + al) * (bh + bl)).sum())
    sab = int((a * b).sum())
    assert 4096 * HH + 64 * (SS - HH - LL) + LL == sab
    assert 2 ** 31 < sab < 2 ** 39 and sab <= 161 * 161 * 4095 * 4095
    assert max(HH, LL) <= 161 * 161 * 63 * 63 < 2 ** 27 and SS <= 161 * 161 * 126 * 126 < 2 ** 29
    # the row-box sums: q in three byte planes, q^2 in a u32 (four byte planes); the box sums of q in an i32
    assert a.sum(axis=1).max() < 2 ** 20 and 2 ** 31 < (a * a).sum(axis=1).max() < 2 ** 32 and a.sum() < 2 ** 27
    # the finish: n sum ab and (sum a)^2 pass 2^53 here -- the products round, in the float kernel's own operations
    assert 161 * 161 * sab > 2 ** 53


@pytest.mark.parametrize("period", wp.SEAM_PERIODS)
def test_seam_pairs_tie_across_tiles(period):
    """the oracle's own facts on the 12-bit pairs: the maxima are exactly tied, lie in different tiles, and the first in k wins"""
    p0, p1, xy = wp.seam_pair(*period, plateau=False)
    assert p0.max() > 255 and np.array_equal(p0[:, :-period[0]], p0[:, period[0]:]) and np.array_equal(p0[:-period[1]], p0[period[1]:])
    rec, cand, surf, nlm = full_any(p0, p1, xy[:2], (0, 0), wp.SEAM_OCW, wp.SEAM_R, 8)
    S = 2 * wp.SEAM_R + 1
    xs, ys = wp.maxima_cells(period[0]), wp.maxima_cells(period[1])
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


@pytest.mark.parametrize("R,y", wp.SEAM_PLATEAUS)
def test_seam_plateau(R, y):
    p0, p1, xy = wp.seam_pair(*wp.PLATEAU_PERIOD, plateau=True)
    rec, cand, surf, nlm = full_any(p0, p1, xy[:1], (0, 0), wp.SEAM_OCW, R, 8)
    S = 2 * R + 1
    v = surf[0].reshape(S, S)
    assert (y + 1) % 32 == 0 and v[R, y] == v[R, y + 1] and v[R, y] == v.max()


def test_far_pair_is_within_reach_of_both_chip_sizes():
    c = far_case()
    for ocw in (16, 10):
        rec, _, _, _ = full_any(spread12(c.i0), spread12(c.i1), c.xyuvav, (0, 0), ocw, FAR_R, 0)
        assert np.isfinite(rec[:, 0]).all()
        assert np.hypot(rec[:, 0] - FAR_TRUE[0], rec[:, 1] - FAR_TRUE[1]).max() < 0.5
