"""CPU: the facts the GPU tests of mimc3_match_ncc_wide_chip (tests/test_wide_chip.py) rely on -- the new symbols, the library's layout
and dispatch table against their restatements in tests/wide_chip_common.py, every GPU fixture qualified on the oracle, and the judge
rejecting the two results the kernel could produce by mistake without a value test of one tile noticing."""
import numpy as np
import pytest

import wide_chip_common as wc
from full_chip_common import BAND_SHAPES


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def test_symbols_exist(api):
    for name in wc.SYMBOLS:
        assert hasattr(api._lib, name), name
    for name in ("match_ncc_wide_chip", "match_ncc_wide_chip_dev"):
        assert hasattr(api.Context, name), name
    for name in ("wide_chip_max_radius", "wide_chip_layout", "wide_chip_path"):
        assert hasattr(api, name), name


def test_layout_matches_the_library(api):
    for ocw in range(1, wc.MAX_OCW + 1):
        assert api.wide_chip_max_radius(ocw) == wc.R_MAX
        for R in range(wc.R_MIN, wc.R_MAX + 1):
            got = api.wide_chip_layout(ocw, R)
            assert got == wc.layout(ocw, R), (ocw, R, got)
            ntx, br, nb, wgs, lds = got
            cw = 2 * ocw + 1
            assert lds + wc.STATIC_BYTES <= wc.CU_LDS and 1 <= br <= cw and nb * br >= cw and (nb - 1) * br < cw, (ocw, R, got)
            assert ntx == -(-(2 * R + 1) // 32) and wgs >= 1 and wgs * (lds + wc.STATIC_BYTES) <= wc.CU_LDS, (ocw, R, got)
            # two workgroups per CU wherever the whole chip is then one band; else the tallest band one workgroup holds
            if nb > 1:
                assert wgs == 1 and wc.layout_full(ocw, R)["lds"] + 4 * (wc.layout_full(ocw, R)["PB"] + wc.layout_full(ocw, R)["CWP"]) + wc.STATIC_BYTES > wc.CU_LDS
    for ocw, R in ((0, 16), (81, 16), (10, 15), (10, 48)):
        assert api.wide_chip_layout(ocw, R) is None and wc.layout(ocw, R) is None
    assert api.wide_chip_max_radius(0) == 0 and api.wide_chip_max_radius(81) == 0
    # the largest chip at the largest radius: about 63 KB for one band row, the 31 shared rows and the surface
    L = wc.layout_full(80, 47)
    assert 4 * 32 * L["PB"] + 4 * L["CWP"] + 95 * 96 * 4 < 64 * 1024


def test_path_matches_the_table(api):
    for cls in range(4):
        for ocw in range(0, 82):
            for R in range(0, 49):
                for mode in range(0, 3):
                    assert api.wide_chip_path(cls, ocw, R, mode) == wc.path(cls, ocw, R, mode, api.wide_planes_max_radius), (cls, ocw, R, mode)
    assert api.wide_chip_path(-1, 10, 20, 1) == -1 and api.wide_chip_path(4, 10, 20, 1) == -1
    for ocw in wc.SIX:
        assert api.wide_max_radius(ocw) == wc.WIDE_MAX[ocw]
    # the calls that are refused elsewhere: a 16-bit or float pair at the reference's other chip sets, ocw 40 beyond R 39, 12 bits at ocw 80
    for ocw in (10, 11, 14, 60, 80):
        assert api.wide_chip_path(2, ocw, 16, 0) == api.wide_chip_path(3, ocw, 47, 0) == 16
    assert api.wide_chip_path(2, 40, 39, 0) == 10 and api.wide_chip_path(2, 40, 40, 0) == 16
    assert api.wide_chip_path(1, 80, api.wide_planes_max_radius(80), 0) == 15 and api.wide_chip_path(1, 80, api.wide_planes_max_radius(80) + 1, 0) == 16


def test_band_shapes_in_range():
    """which of the band shapes the layout has at all: a chip is an odd number of rows and a multi-band chip's band is at least 71 rows
    (ocw 80, R 47), so a last band as tall as the others (CW = k BR) cannot occur"""
    found = wc.band_shape_cases(wc.layout)
    assert set(found) == set(BAND_SHAPES) - {"full_last_band"}, found
    assert min(wc.layout(o, r)[1] for o in range(1, 81) for r in range(16, 48) if wc.layout(o, r)[2] > 1) == 71


@pytest.mark.parametrize("fx", wc.all_fixtures(), ids=lambda fx: "-".join(str(x) for x in fx))
def test_fixture_is_qualified(fx):
    """fitted, -3 and -4 points on the oracle; a point with a clean and a masked (tile, band) in one surface"""
    f = wc.fixture(*fx)
    pts, rec, surf = wc.oracle(*fx)
    st = rec[:, 2]
    assert (st == -3).sum() >= 1 and (st == -4).sum() >= 1 and np.isfinite(rec[:, 0]).sum() >= 2, (f["what"], st.tolist())
    assert rec[pts.index(wc.G4), 2] == -4 and rec[pts.index(wc.G3CHIP), 2] == -3
    mixed = 0
    for i, g in enumerate(pts):
        if st[i] == -3:
            continue
        cls = wc.tile_band_classes(f, g)
        mixed += bool(cls.any() and not cls.all())
        if g == wc.BOX_ONLY[1]:         # a null in the box's last column alone: the last tile column is masked, no other
            assert cls[:, -1].any() and not cls[:, :-1].any(), f["what"]
        if g == wc.CHIP_ONLY[0]:        # a null in the first chip row alone: the first band of every tile
            assert cls[:, :, 0].all() and not cls[:, :, 1:].any(), f["what"]
        if g == wc.BOX_ONLY[0]:         # a null in the last box row alone: the last band of the last tile row
            assert cls[-1, :, -1].any() and not cls[:-1].any(), f["what"]
        if g == wc.OUTSIDE:             # a null one column outside the box: no body sees it
            assert not cls.any(), f["what"]
    assert mixed >= 1, f["what"]
    if f["status"]:
        i8, i9, i11 = pts.index(wc.G3BOX), pts.index(wc.CLEAN), pts.index(wc.ONE_TILE)
        assert st[i8] == -3 and st[i9] != -3 and st[i11] == -2 and not np.isfinite(surf[i11]).any()
        u, v, cu, cv = (a[wc.CLEAN] for a in f["geo"])
        h = f["ocw"] + f["R"]
        share = (f["i1"][cv - h:cv + h + 1, cu - h:cu + h + 1] == 0).mean()
        assert 0.45 < share < 0.8


def test_judge_rejects_a_shifted_tile_and_a_per_tile_count():
    fx = wc.STATUS
    f = wc.fixture(*fx)
    pts, rec, surf = wc.oracle(*fx)
    R, S = f["R"], 2 * f["R"] + 1
    xy, sh = wc.sub(f, pts)
    wc.judge((rec.copy(), None, surf.copy()), rec, surf, sh, R, 0, True, "the oracle itself")
    # the second tile column taken from a window one pixel aside: cells x = 32 .. 63 are those of x + 1
    bad = surf.copy().reshape(-1, S, S)                     # [point][x][y]
    bad[:, 32:64] = surf.reshape(-1, S, S)[:, 33:65]
    with pytest.raises(AssertionError):
        wc.judge((rec.copy(), None, bad.reshape(surf.shape)), rec, surf, sh, R, 0, True, "shifted tile")
    # a status decided from a box null count taken once per tile: the 60 % box, counted in every tile's window, is refused
    i9 = pts.index(wc.CLEAN)
    u, v, cu, cv = (a[wc.CLEAN] for a in f["geo"])
    h = f["ocw"] + f["R"]
    nulls = f["i1"][cv - h:cv + h + 1, cu - h:cu + h + 1] == 0
    ntx, cw = wc.layout(f["ocw"], R)[0], 2 * f["ocw"] + 1
    per_tile = sum(int(nulls[32 * ty:32 * ty + cw + 31, 32 * tx:32 * tx + cw + 31].sum()) for ty in range(ntx) for tx in range(ntx))
    assert np.float32(per_tile) / np.float32(nulls.size) > np.float32(0.8) and rec[i9, 2] != -3
    rec3, surf3 = rec.copy(), surf.copy()
    rec3[i9] = np.nan; rec3[i9, 2] = -3
    surf3[i9] = np.nan
    with pytest.raises(AssertionError):
        wc.judge((rec3, None, surf3), rec, surf, sh, R, 0, True, "per-tile count")
