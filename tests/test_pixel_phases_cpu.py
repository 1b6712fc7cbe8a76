"""CPU: the fixtures of tests/phase_common.py qualified -- they reach every pixel phase of chip and window origin with every null class,
on every list of the matrix-core step; the oracles truncate fractional coordinates as the reference does; and a record of which phases
the older fixtures reach.  tests/test_pixel_phases.py runs the kernels on what is qualified here."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from mimc3_amd import api, synth
from phase_common import (BRIGHT_POINTS, DIMX, KINDS, OCWS, OFFSETS, SEARCH_R, coverage, coverage_table, fixture, fractional, geometry, phases,
                          search_shifts, trunc)
from value_limit_common import local_ranges

U_OFFSETS = OFFSETS[:4]           # the coverage conditions hold over the four offsets in u alone


# ---- the coverage condition: a condition on the fixture.  If it does not hold, change the fixture, never the condition. ----------------
@pytest.mark.parametrize("ocw", OCWS)
def test_every_phase_cell_holds_every_null_class(ocw):
    f = fixture(ocw)
    cells = coverage(f, "dlc", offsets=U_OFFSETS)
    print(coverage_table(f, "dlc"))
    for cph in range(4):
        for wph in range(4):
            for dx4 in (1, 3):
                for null in range(4):
                    assert cells[(cph, wph, dx4, null)] >= 1, (cph, wph, dx4, null)
    cells16 = coverage(f, "dlc16", offsets=U_OFFSETS)
    assert all(cells16[(a, b, dx4, null)] >= 1 for a in (0, 1) for b in (0, 1) for dx4 in (1, 3) for null in range(4))


@pytest.mark.parametrize("ocw", OCWS)
def test_every_phase_pair_occurs_on_every_list_of_the_matrix_core_step(ocw):
    f = fixture(ocw)
    cells = coverage(f, "auto", offsets=U_OFFSETS)
    print(coverage_table(f, "auto"))
    assert all(cells[(a, b, lst)] >= 1 for a in range(4) for b in range(4) for lst in ("clean", "advance", "rest"))


@pytest.mark.parametrize("ocw,radius", [(ocw, SEARCH_R) for ocw in OCWS] + [(7, 15), (40, 15)])
def test_every_phase_pair_occurs_with_every_null_class_in_the_searches(ocw, radius):
    f = fixture(ocw, plan="search")
    cells = coverage(f, "search", radius=radius, offsets=U_OFFSETS)
    assert all(cells[(a, b, null)] >= 1 for a in range(4) for b in range(4) for null in range(4))


@pytest.mark.parametrize("ocw", OCWS)
def test_the_fixture_is_what_its_docstring_says(ocw):
    f = fixture(ocw)
    H, W = f.i0.shape
    assert H <= 1000 and W <= 1000 and f.xy.shape[0] <= 100
    su, sv = geometry(ocw)[4:]
    assert su % 2 == 1 and sv % 2 == 1
    last = f.uv[f.off[1:] - 1]
    assert su > 2 * (np.abs(last[:, 0]).max() + ocw + 2) + 1 + 4 and sv > 2 * (np.abs(last[:, 1]).max() + ocw + 2) + 1 + 4      # windows apart
    assert set((np.abs(last[:, 0]) & 1).tolist()) == {0, 1}
    assert np.array_equal(np.bincount(f.cls, minlength=4), [16, 16, 16, 16])
    for plan in ("dlc", "search"):
        assert int((fixture(ocw, plan=plan).i0 == 0).sum()) == 32 and int((fixture(ocw, plan=plan).i1 == 0).sum()) == 32      # one pixel each
    for plan in ("dlc", "search"):                              # every pixel class: the same nulls, so the same cells, in both plans
        f8 = fixture(ocw, plan=plan)
        for kind in KINDS[1:]:
            g = fixture(ocw, kind, plan=plan)
            assert np.array_equal(g.i0 == 0, f8.i0 == 0) and np.array_equal(g.i1 == 0, f8.i1 == 0) and np.array_equal(g.uv, f8.uv)
            assert np.array_equal(g.xy, f8.xy) and np.array_equal(g.off, f8.off)
    # 9-bit: the chip or the window of every 16th point spans more than a byte, at every offset and in both directions, so those points
    # leave the u8 kernels' offset scheme for the u16 list; no other point's does
    g = fixture(ocw, "9bit")
    for offset in OFFSETS:
        for i0, i1, sgn in ((g.i0, g.i1, 1), (g.i1, g.i0, -1)):
            rc, rw = local_ranges(i0, i1, g.xy, sgn * np.asarray(offset), g.off, sgn * g.uv, ocw)
            assert np.array_equal(np.flatnonzero((rc > 254) | (rw > 254)), BRIGHT_POINTS), (offset, sgn)
    top = {"u8": 255, "9bit": 500, "12bit": 4095, "eighths": 4095 / 8, "16bit": 65535}
    for kind in KINDS:
        g = fixture(ocw, kind)
        assert top[kind] / 2 < max(g.i0.max(), g.i1.max()) <= top[kind], kind


# ---- fixture sanity on the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocw", OCWS)
def test_points_are_valid_and_a_chip_moved_by_one_pixel_changes_every_record(oracle, ocw):
    """a staging that is off by one phase reads the chip or the window one to three pixels aside: that cannot pass if one pixel already
    changes every valid point's record"""
    f = fixture(ocw)
    for offset in (OFFSETS[0], OFFSETS[3]):
        want = oracle.match(f.i0, f.i1, f.xy, offset, f.off, f.uv, ocw)
        valid = want[:, 2] > -2.5
        assert valid.mean() > 0.5
        for moved, what in ((np.roll(f.i0, 1, axis=1), "chip"), (np.roll(f.i1, 1, axis=1), "window")):
            other = oracle.match(moved, f.i1, f.xy, offset, f.off, f.uv, ocw) if what == "chip" else \
                oracle.match(f.i0, moved, f.xy, offset, f.off, f.uv, ocw)
            same = (np.nan_to_num(other).view(np.uint32) == np.nan_to_num(want).view(np.uint32)).all(axis=1)
            assert not (same & valid).any(), f"{what} moved by one pixel: points {np.flatnonzero(same & valid).tolist()} keep their record"


def test_search_records_change_with_a_chip_moved_by_one_pixel():
    from full_search_common import full_search
    f = fixture(16, plan="search")
    shift = search_shifts(f)[0]
    want = full_search(f.i0, f.i1, f.xy, (1, 0), 16, SEARCH_R, shift=shift)
    other = full_search(np.roll(f.i0, 1, axis=1), f.i1, f.xy, (1, 0), 16, SEARCH_R, shift=shift)
    valid = want[:, 2] > -2.5
    assert valid.mean() > 0.5
    assert not ((np.nan_to_num(other).view(np.uint32) == np.nan_to_num(want).view(np.uint32)).all(axis=1) & valid).any()


# ---- truncation (MIMC_module.c:822-823) ---------------------------------------------------------------------------------------
def test_fractional_grid_keeps_the_truncated_coordinates_and_holds_every_fraction():
    f = fixture(7)
    for seed in range(3):
        fr = fractional(f.xy, seed)
        assert np.array_equal(trunc(fr)[0], trunc(f.xy)[0]) and np.array_equal(trunc(fr)[1], trunc(f.xy)[1])
        pairs = {(round(a - np.trunc(a), 6), round(b - np.trunc(b), 6)) for a, b in fr[:, 2:4]}
        assert len(pairs) == 25                                 # every fraction of u with every fraction of v
        # 1 - 2^-20 is below the next integer in f64 and rounds up to it in f32 from 16 on: a site that truncates (int)(float)u is a pixel off
        assert (fr[:, 2:4] < np.trunc(fr[:, 2:4]) + 1).all()
        assert (fr[:, 2:4].astype(np.float32) == np.trunc(fr[:, 2:4]) + 1).any()
        p, q = phases(f.xy, (1, 0), f.off, f.uv, 7), phases(fr, (1, 0), f.off, f.uv, 7)
        assert all(np.array_equal(p[k], q[k]) for k in p)


@pytest.mark.parametrize("ocw", [7, 16])
def test_the_oracles_truncate(oracle, ocw):
    from full_any_common import full_any
    from full_dn_common import full_dn
    from full_multi_common import full_multi
    from full_search_common import full_search
    f = fixture(ocw, plan="search")
    H, W = f.i0.shape
    fr = fractional(f.xy, 1)
    off, uv = oracle.get_uv_pivot(fr, f.dt, f.mpp, ocw, H, W)
    assert np.array_equal(off, f.off) and np.array_equal(uv, f.uv)       # (far from the edges the corridor does not see the fraction)
    shift = search_shifts(f)[0]
    assert np.array_equal(api.prior_shift(fr, f.dt, f.mpp), shift)
    offset = (1, -1)
    assert_bits_equal(oracle.match(f.i0, f.i1, fr, offset, off, uv, ocw), oracle.match(f.i0, f.i1, f.xy, offset, off, uv, ocw), "match")
    assert_bits_equal(full_search(f.i0, f.i1, fr, offset, ocw, SEARCH_R, shift=shift),
                      full_search(f.i0, f.i1, f.xy, offset, ocw, SEARCH_R, shift=shift), "full_search")
    for name, fn in (("full_multi", full_multi), ("full_dn", full_dn), ("full_any", full_any)):
        a, b = fn(f.i0, f.i1, fr, offset, ocw, SEARCH_R, 4, shift=shift), fn(f.i0, f.i1, f.xy, offset, ocw, SEARCH_R, 4, shift=shift)
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"{name}, result {k}"


def test_the_pyramid_oracles_truncate():
    from pyramid_any_oracle import pyramid_search_any
    from pyramid_dn_oracle import pyramid_search_dn
    from pyramid_oracle import pyramid_search
    f = fixture(7, plan="search")
    fr = fractional(f.xy, 2)
    shift = search_shifts(f)[0]
    a, b = pyramid_search(f.i0, f.i1, fr, (1, -1), 7, SEARCH_R, 2, shift=shift), pyramid_search(f.i0, f.i1, f.xy, (1, -1), 7, SEARCH_R, 2, shift=shift)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    g = fixture(7, "16bit", plan="search")
    for fn in (pyramid_search_dn, pyramid_search_any):
        a, b = fn(g.i0, g.i1, fr, (1, -1), 7, SEARCH_R, 2, 4, shift=shift), fn(g.i0, g.i1, g.xy, (1, -1), 7, SEARCH_R, 2, 4, shift=shift)
        for k in range(3):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{fn.__name__}, result {k}"


def edge_points(ocw, H, W):
    """points whose corridor meets the image's edge at a fraction: get_uv_pivot compares u + (float)row[2] -+ ocw with 0 and W - 1
    untruncated (MIMC_module.c:576-585), so there the fraction counts"""
    us = [ocw + 0.9, ocw + 0.25, ocw + 1.0, W - 1 - ocw - 0.1, W - 1 - ocw - 0.75, W - 2 - ocw + 0.5, W / 2 + 0.5]
    vs = [ocw + 0.9, H - 1 - ocw - 0.1, H / 2 + 0.75]
    rows = []
    for k, u in enumerate(us):
        for j, v in enumerate(vs):
            ang = np.deg2rad(40.0 * (k * len(vs) + j))
            rows.append([u * synth.MPP, -v * synth.MPP, u, v, 1500.0 * np.cos(ang), 1500.0 * np.sin(ang)])
    return np.ascontiguousarray(rows, np.float64)


@pytest.mark.parametrize("ocw", [7, 40])
def test_pivots_of_fractional_points_vs_reference(oracle, reference, ocw):
    f = fixture(ocw)
    H, W = f.i0.shape
    for xy in (fractional(f.xy, 0), edge_points(ocw, H, W)):
        a, b = reference.get_uv_pivot(xy, f.dt, f.mpp, ocw, H, W), oracle.get_uv_pivot(xy, f.dt, f.mpp, ocw, H, W)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = api.get_uv_pivot(xy, f.dt, f.mpp, ocw, H, W)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert_bits_equal(reference.match(f.i0, f.i1, fractional(f.xy, 0), (2, 1), f.off, f.uv, ocw),
                      oracle.match(f.i0, f.i1, f.xy, (2, 1), f.off, f.uv, ocw), "the reference on the fractional grid vs the oracle on the truncated one")


# ---- a record of the gap ------------------------------------------------------------------------------------------------------------------
def test_the_older_fixtures_reach_few_phases():
    """Which u0 mod 4 the regular grids of the older fixtures hold -- why tests/phase_common.py exists.  At ocw 30 and 40 the small
    fixtures of tests/test_match_parity.py and tests/null_encoding_common.py hold no odd chip column, and each BASELINE configuration
    holds one u0 mod 4.  This records the state of those fixtures when the phase tests were written, nothing the product must keep: if
    someone later changes those fixtures so that this fails, delete this test, do not bend it."""
    from null_encoding_common import GEOM
    from test_match_parity import SMALL

    def u_mod4(xy):
        return set((trunc(xy)[0] & 3).tolist())

    small = {k["seed"]: u_mod4(synth.make_small(**k).xyuvav) for k in SMALL}
    assert small[31] == {1} and small[38] == {1} and small[39] == {1}
    assert small[36] == {0, 2} and small[42] == {0} and small[37] == {0, 2}
    geom = {ocw: u_mod4(synth.make_small(ocw=ocw, **kw).xyuvav) for ocw, kw in GEOM.items()}
    assert geom[7] == {1} and geom[30] == {0, 2} and geom[40] == {0, 2} and geom[15] == {1}
    for k in SMALL:
        if k["ocw"] in (30, 40):
            assert not any(u & 1 for u in small[k["seed"]])
    want = {"C1": {2}, "C2": {0}, "C4": {0}}
    for name, phase in want.items():
        h, w, dimx, dimy, u0, v0, su, sv = synth._CONFIGS[name][:8]
        assert u_mod4(synth.make_grid(dimx, dimy, u0, v0, su, sv, 1806.0)) == phase, name
    assert all(len(u_mod4(grid_of.xy)) == 4 for grid_of in (fixture(ocw) for ocw in OCWS))        # and the new ones hold all four
    assert DIMX >= 8
