"""The clean form's window-side box sums from the window plane's packed table (match_mx_kernel.hip, RecCfg<OCW, true>; sat_cell_corners,
sat_kernel.h) on the GPU, at all six chip sizes: small pairs of about 30 points, every call the CPU oracle's bit for bit and the same
bytes as the same call with MIMC3_MX_BOX_TABLE=0 (the MFMA box sums), on the matrix-core path (last_path() == "u8_mfma", asserted in
the child processes of tests/u8_advance_common.advance_stats), with the same list figures of MIMC3_MX_STATS -- no point changes route.

  (a) peaks on the last reachable column, the last reachable row and their corner: the pair's shift lies one cell beyond the last pivot,
      in both flow directions (with the flow the far edge is the cells next to the never-written last column / row, T4, where the
      clamp of the far corner decides; against it the first reachable cells);
  (b) points whose window leaves the image while their chip stays inside: advance points at the image edge;
  (c) advance points with nulls elsewhere in the window (u8_advance_common.blobs_case, t4_case);
  (d) axis-aligned flow: an area of five rows, most bands skipped;
  (e) ocw 40: a saturated pair, every pixel 254 or 255.

What each fixture holds is counted with the rule restated in numpy (u8_advance_common.classify, test_mx_area_finish's areas, bands and
speculative climbs) and asserted, not assumed."""
import functools

import numpy as np
import pytest

import test_mx_area_finish as af
import u8_advance_common as ac
from conftest import assert_bits_equal

OCWS = (7, 15, 16, 30, 32, 40)
FLOW = ((1, 1), (-1, -1))
LU, LV = 6, 4                      # |last pivot| of the hand-made fixtures: a 16 x 12 cell grid, the tile at origin 1 holds all of it
EDGES = ("column", "row", "corner")


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line_case(ocw, lu, lv, shift, margin=None, seed=0):
    """30 points on a null-free pair, every point with the pivots of the line from (0, 0) to (lu, lv)"""
    c = ac.small(ocw, 9300 + ocw + seed, shift=shift, margin=ocw + 42 if margin is None else margin)
    xy = np.ascontiguousarray(c.xyuvav).copy()
    piv = af.line_pivots(lu, lv)
    off = np.arange(len(xy) + 1, dtype=np.int64) * len(piv)
    return c.i0, c.i1, xy, np.zeros(2, np.int32), off, np.ascontiguousarray(np.tile(piv, (len(xy), 1)), np.int32), ocw


def far_edge_case(ocw, sx, sy, edge):
    lu, lv = sx * LU, sy * LV
    shift = (lu + (sx if edge != "row" else 0), lv + (sy if edge != "column" else 0))
    return line_case(ocw, lu, lv, shift, seed=10 * EDGES.index(edge) + (sx > 0))


def image_edge_case(ocw, sx, sy):
    return line_case(ocw, sx * LU, sy * LV, (3 * sx, 2 * sy), margin=ocw + 3, seed=40 + (sx > 0))


def axis_case(ocw):
    return line_case(ocw, 8, 0, (3, 0), seed=50)


def saturated_case(ocw):
    i0, i1, *rest = line_case(ocw, LU, LV, (3, 2), seed=60)
    return (np.where(i0 > np.median(i0), 255.0, 254.0).astype(np.float32), np.where(i1 > np.median(i1), 255.0, 254.0).astype(np.float32), *rest)


def named_cases(api, ocw):
    cases = [("far %s flow %s" % (e, f), far_edge_case(ocw, f[0], f[1], e)) for f in FLOW for e in EDGES]
    cases += [("image edge flow %s" % (f,), image_edge_case(ocw, *f)) for f in FLOW]
    # (at ocw 40 the blobs fixture as it stands has no advance point -- its 113-pixel windows all hold a blob near the area: another draw)
    blobs = ac.blobs_case(api, ocw) if ocw < 40 else ac.blobs_case(api, ocw, seed=8861, null_frac=0.01)
    cases += [("blobs", blobs), ("t4", ac.t4_case(api, ocw)), ("axis", axis_case(ocw))]
    if ocw == 40:
        cases.append(("saturated", saturated_case(ocw)))
    return cases


def case_list(api, ocw):
    return [c for _, c in named_cases(api, ocw)]


# ---- what a fixture holds, in numpy ------------------------------------------------------------------------------------------------------
def some_climb_reads(case, want_x, want_y):
    """some clean point has a scan of its speculative climbs that reads cell column want_x (None: any) and cell row want_y"""
    a = af.areas(case)
    for g in np.flatnonzero(a["clean"]):
        for centres, _, _ in af.speculative_climbs(case, g):
            for cx, cy in centres:
                if (want_x is None or abs(cx - want_x) <= 1) and (want_y is None or abs(cy - want_y) <= 1):
                    return True
    return False


def check_kind(name, case, ocw):
    i0, i1, xy, offset, off, uv, _ = case
    k = ac.classify(i0, i1, xy, offset, off, uv, ocw)
    if name.startswith("far") or name in ("axis", "saturated"):
        assert k["clean"].all(), name
    if name.startswith("far"):
        with_flow = "(1, 1)" in name
        # the cells a climb reads at the far edge: with the flow the T4 column / row cs - 2, against it the first reachable cell 1
        ex, ey = (2 * LU + 4, 2 * LV + 4) if with_flow else (1, 1)
        assert some_climb_reads(case, None if "row" in name else ex, None if "column" in name else ey), name
    elif name.startswith("image edge"):
        H, W = i0.shape
        leaves = (k["wu"] < 0) | (k["wv"] < 0) | (k["wu"] + 2 * k["dx2"] + 1 > W) | (k["wv"] + 2 * k["dy2"] + 1 > H)
        u0, v0 = xy[:, 2].astype(np.int64), xy[:, 3].astype(np.int64)
        assert ((u0 - ocw >= 0) & (u0 + ocw < W) & (v0 - ocw >= 0) & (v0 + ocw < H)).all(), name
        assert int((k["advance"] & leaves).sum()) >= 1 and int((k["clean"] & ~leaves).sum()) >= 1, name
    elif name in ("blobs", "t4"):
        assert int(k["advance"].sum()) >= 1 and int(k["clean"].sum()) >= 1, (name, ocw)
    elif name == "axis":
        b = af.bands(af.areas(case))
        assert all(bin(int(v)).count("1") <= 2 for v in b[:, 0]) and (b[:, 0] != 0).all(), name      # five rows: at most two of the eight bands
    elif name == "saturated":
        assert min(i0.min(), i1.min()) == 254 and max(i0.max(), i1.max()) == 255


def test_fixtures_hold_their_kind():
    """without a GPU, at the two chip sizes where the restated climbs take a second"""
    from mimc3_amd import api
    for ocw in (7, 16):
        for name, case in named_cases(api, ocw):
            check_kind(name, case, ocw)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_table_box_sums(api, oracle, tmp_path, ocw):
    named = named_cases(api, ocw)
    for name, case in named:
        check_kind(name, case, ocw)
    body = "import test_mx_box_table as t; cases = t.case_list(api, %d)" % ocw
    on = ac.advance_stats(body, outdir=str(tmp_path / "on"))
    off = ac.advance_stats(body, env={"MIMC3_MX_BOX_TABLE": "0"}, outdir=str(tmp_path / "off"))
    assert len(on) == len(off) == len(named)
    finished = 0
    for i, (name, case) in enumerate(named):
        i0, i1, xy, offset, off_, uv, _ = case
        got = np.load(tmp_path / "on" / f"{i}.npy")
        assert_bits_equal(got, oracle.match(i0, i1, xy, offset, off_, uv, ocw), f"ocw {ocw} {name}: table box sums vs oracle")
        assert_bits_equal(got, np.load(tmp_path / "off" / f"{i}.npy"), f"ocw {ocw} {name}: table vs MFMA box sums")
        print("ocw", ocw, name, "(clean list, rest list, finished, rest after, advance list, tried, finished):", on[i], "| switch off:", off[i])
        assert on[i] == off[i], (ocw, name)                                       # no point changes route
        finished += on[i][2] + on[i][6]
        if name.startswith("far") or name in ("axis", "saturated"):
            assert on[i][2] >= 1, (ocw, name)                                     # the matrix-core launch itself finishes clean points of it
        if name.startswith("image edge") or name in ("blobs", "t4"):
            assert on[i][5] == on[i][4] >= 1, (ocw, name)                         # ... and tries its advance points
        if name.startswith("image edge"):
            assert on[i][6] >= 1, (ocw, name)                                     # ... and finishes some
    # (an advance point whose climb leaves its area is left to the register-tiled launch -- the t4 fixture's only one at ocw 15: between
    #  them the two null fixtures have advance points the matrix-core launch finishes)
    assert sum(on[i][6] for i, (name, _) in enumerate(named) if name in ("blobs", "t4")) >= 1, ocw
    assert finished > 0
