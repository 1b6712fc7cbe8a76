"""The clean form's area finish (match_mx_kernel.hip, u8_classify_kernel.hip): clean points carry their climb area (mx_climb_area,
match_kernel.h), the NCC finish runs only over the bands of four tile rows that meet it, and a clean point whose climb leaves the area is
handed to the register-tiled launch.  Every output is compared bit for bit against the CPU oracle, forward and swapped; the list figures
(clean list, finished, rest list before and after) come from the kernels' diagnostics in a child process (tests/u8_advance_common.py).

The fixtures are null-free pairs of about (2 ocw + 250)^2 pixels with 20 points and hand-made pivot lists along a line from (0, 0) to the
last pivot, so that the last pivot -- and with it the area's place in the tile -- is chosen per point.  What they reach is stated in
numpy and asserted without a GPU (test_fixture_geometry): the four sign combinations of the last pivot, every residue mod 4 of the area's
first and last row, T4 rows inside the area and in a skipped band, wave 1's columns skipped, every byte phase of chip and window origin.
Not reachable: wave 0's columns skipped (the area always holds pivot (0, 0)'s cell, which lies in the tile's first 16 columns).

The speculative climb of the kernel (every pivot, up to 16 scans, ignoring the visited state) is restated in numpy on the exact f32
surfaces: it predicts which clean points stay inside their area, without a GPU (test_climbs_stay_inside_the_area) and as the exact
hand-on count on one (the GPU tests)."""
import functools

import numpy as np
import pytest

import ncc_edge_common as ec
import phase_common as pc
import u8_advance_common as ac
from conftest import assert_bits_equal
from mimc3_amd import synth

OCWS = (7, 16)
DIRECTIONS = ((1, -1), (-1, -1), (1, 1), (-1, 1))          # signs of the last pivot (and of the true shift)
OFFSETS = ((0, 0), (1, 0), (2, 0), (3, 1))                 # the four window phases in u, two in v (the grid's jitter moves v as well)
LV = (5, 6, 7, 8, 9, 10, 11, 12)                           # |lv| by point: four consecutive residues, twice; |lu| = round(1.5 |lv|) = 8 .. 18
SPEC_ROUNDS = 16                                           # kSpecRounds
RESTATED = {7: OFFSETS, 16: (OFFSETS[0], OFFSETS[3])}      # where the climbs are restated in numpy (a second or two per chip size)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def line_pivots(lu, lv):
    n = max(abs(lu), abs(lv))
    return np.array([(int(round(k * lu / n)), int(round(k * lv / n))) for k in range(n + 1)], np.int32)


@functools.lru_cache(maxsize=None)
def direction_case(ocw, sx, sy, offset=(0, 0)):
    """20 points, last pivots (sx round(1.5 m), sy m) for m in LV by turns, the pair's shift such that the peak lies at (3 sx, 2 sy) from
    the offset, on every point's line; u0, v0 jittered so that one launch holds all four chip phases in both axes"""
    c = synth.make_small(seed=9100 + ocw + 10 * (sx + 1) + 3 * (sy + 1), ocw=ocw, shift=(3 * sx + offset[0], 2 * sy + offset[1]), angle_deg=40.0, speed=1700.0, noise_dn=2,
                         null_frac=0.0, h=2 * ocw + 250, w=2 * ocw + 260, dimx=5, dimy=4, margin=ocw + 42)
    xy = np.ascontiguousarray(c.xyuvav).copy()
    g = np.arange(len(xy))
    xy[:, 2] = (np.trunc(xy[:, 2]).astype(np.int64) & ~3) + (g & 3)
    xy[:, 3] = (np.trunc(xy[:, 3]).astype(np.int64) & ~3) + ((g >> 2) & 3)
    lists = [line_pivots(sx * int(round(1.5 * LV[i % len(LV)])), sy * LV[i % len(LV)]) for i in g]
    off = np.zeros(len(xy) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in lists])
    return c.i0, c.i1, xy, np.asarray(offset, np.int32), off, np.ascontiguousarray(np.concatenate(lists), np.int32), ocw


def off_corridor_case(api, ocw):
    """ac.off_corridor_case's recipe without nulls: 17 to 29 pivots, the shift far off the corridor"""
    c = ac.small(ocw, 8450 + ocw, null_frac=0.0, shift=(9, 7), angle_deg=45.0, speed=2900.0, h=2 * ocw + 300, w=2 * ocw + 310, dimx=6, dimy=6,
                 margin=ocw + 80)
    off, uv = ac.pivots(api, c, ocw)
    return c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw


def edge_case(ocw):
    """the rounding-boundary fixture of this chip size, as it stands (its clean points are the ones the clean form finishes)"""
    (path,) = [p for p in ec.fixture_paths() if p.endswith("ocw%02d.npz" % ocw)]
    f = ec.load(path)
    return f["i0"], f["i1"], f["xyuvav"], f["offset"], f["piv_off"], f["piv_uv"], ocw, f["targets"]


# ---- the rule and the climb, restated ----------------------------------------------------------------------------------------------------
def areas(case):
    """per point: tile origin (tx0, ty0), the area's tile-relative bounds (x0, x1, y0, y1), cs - 2 per axis; and ac.classify's classes"""
    i0, i1, xy, offset, off, uv, ocw = case[:7]
    k = ac.classify(i0, i1, xy, offset, off, uv, ocw)
    last = np.asarray(uv)[np.asarray(off)[1:] - 1].astype(np.int64)
    _, tx, ax0, ax1, _, _ = ac.axis_geometry(last[:, 0], ocw)
    _, ty, ay0, ay1, _, _ = ac.axis_geometry(last[:, 1], ocw)
    csx, csy = 2 * np.abs(last[:, 0]) + 6, 2 * np.abs(last[:, 1]) + 6
    return dict(k, tx=tx, ty=ty, x0=ax0 - tx, x1=ax1 - tx, y0=ay0 - ty, y1=ay1 - ty, t4x=csx - 2 - tx, t4y=csy - 2 - ty, last=last)


def bands(a):
    """bit ci of [.., wave]: the finish runs band ci (tile rows 4 ci .. 4 ci + 3) in wave w (tile columns 16 w .. 16 w + 15)"""
    rows = (2 << (a["y1"] >> 2)) - (1 << (a["y0"] >> 2))
    return np.stack([np.where((w >= (a["x0"] >> 4)) & (w <= (a["x1"] >> 4)), rows, 0) for w in (0, 1)], axis=1)


def surface(case, g):
    """the f32 NCC of every cell of point g's compact grid [cy][cx], as the reference computes a cell (:734): exact integer sums over the
    pixels where chip and window are both non-null (the window's never-written last row and column are null), the f64 formula rounded"""
    i0, i1, xy, offset, off, uv, ocw = case[:7]
    cw = 2 * ocw + 1
    lu, lv = (int(v) for v in np.asarray(uv)[off[g + 1] - 1])
    dx2, dy2 = abs(lu) + ocw + 2, abs(lv) + ocw + 2
    u0, v0 = int(xy[g, 2]), int(xy[g, 3])
    wu, wv = u0 + int(offset[0]) - dx2, v0 + int(offset[1]) - dy2
    a = i0[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1].astype(np.float64)
    w = i1[wv:wv + 2 * dy2 + 1, wu:wu + 2 * dx2 + 1].astype(np.float64).copy()
    w[-1, :] = 0
    w[:, -1] = 0
    b = np.lib.stride_tricks.sliding_window_view(w, (cw, cw))
    m = (b != 0) & (a != 0)
    am = np.where(m, a, 0.0)
    n, sx, sxx = m.sum((2, 3)).astype(np.float64), am.sum((2, 3)), (am * am).sum((2, 3))
    bm = np.where(m, b, 0.0)
    sy, syy, sxy = bm.sum((2, 3)), (bm * bm).sum((2, 3)), (am * bm).sum((2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((n * sxy - sx * sy) / np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy))).astype(np.float32)


def speculative_climbs(case, g, val=None):
    """per pivot: the scan centres (compact cells) of its climb on the complete surface, ignoring the visited state, at most 16 scans
    (the kernel's speculation: the real climb is a prefix of it), whether each scan moved, and whether the climb was cut at 16 scans
    while still moving"""
    i0, i1, xy, offset, off, uv, ocw = case[:7]
    val = surface(case, g) if val is None else val
    piv = np.asarray(uv)[off[g]:off[g + 1]]
    dx2, dy2 = abs(int(piv[-1][0])) + ocw + 2, abs(int(piv[-1][1])) + ocw + 2
    Dx2, Dy2 = 2 * dx2 + 1, 2 * dy2 + 1
    climbs = []

    def inside(pu, pv):
        return not (pu - ocw <= 1 or pu + ocw >= Dx2 - 1 or pv - ocw <= 1 or pv + ocw >= Dy2 - 1)

    for a, b in piv:
        pu, pv, smax = int(a) + dx2, int(b) + dy2, np.float32(-2.0)
        alive, centres, moves = inside(pu, pv), [], []
        while alive and len(centres) < SPEC_ROUNDS:
            cx, cy = pu - ocw, pv - ocw
            centres.append((cx, cy))
            v = [val[cy + j % 3 - 1, cx + j // 3 - 1] for j in range(9)]
            m = max(v)
            j = v.index(m)
            moved = bool(m > smax) and j != 4
            smax = max(smax, m)
            moves.append(moved)
            if moved:
                pu, pv = pu + j // 3 - 1, pv + j % 3 - 1
            alive = moved and inside(pu, pv)
        climbs.append((centres, moves, alive))
    return climbs


def stays_inside(case, a, g):
    """the matrix-core launch finishes point g: every scan of its speculative climbs keeps its nine cells inside the area
    (mx_area_scan_bounds), and no climb that was cut at 16 scans really performs all 16 (the replay with the visited cells, pivot by
    pivot: a scan that meets no unvisited cell, or does not move, is a climb's last)"""
    climbs = speculative_climbs(case, g)
    c = np.array([c for centres, _, _ in climbs for c in centres], np.int64).reshape(-1, 2)
    rx, ry = c[:, 0] - a["tx"][g], c[:, 1] - a["ty"][g]
    if not ((rx >= a["x0"][g] + 1) & (rx <= a["x1"][g] - 1) & (ry >= a["y0"][g] + 1) & (ry <= a["y1"][g] - 1)).all():
        return False
    seen = set()
    for centres, moves, cut in climbs:
        t = 0
        for (cx, cy), moved in zip(centres, moves):
            cells = {(cx + i, cy + j) for i in (-1, 0, 1) for j in (-1, 0, 1)}
            fresh = not cells <= seen
            seen |= cells
            t += 1
            if not fresh or not moved:
                break
        if cut and t == len(centres):
            return False
    return True


@functools.lru_cache(maxsize=None)
def ordinary_inside(ocw, sx, sy, offset=(0, 0)):
    case = direction_case(ocw, sx, sy, offset)
    a = areas(case)
    return np.array([stays_inside(case, a, g) for g in range(len(case[2]))])


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------------
def test_fixture_geometry():
    """what the fixtures reach, from the rule restated in numpy"""
    for ocw in OCWS:
        y0r, y1r, t4_in, t4_skipped, wave1_off, origins = set(), set(), 0, 0, 0, set()
        cph, wph = set(), set()
        for sx, sy in DIRECTIONS:
            for o in OFFSETS:
                case = direction_case(ocw, sx, sy, o)
                a = areas(case)
                assert a["clean"].all() and a["takes"].all(), (ocw, sx, sy, o)
                assert (np.sign(a["last"]) == (sx, sy)).all()
                ph = pc.phases(case[2], case[3], case[4], case[5], ocw)
                cph |= set(zip(ph["cph"].tolist(), ph["cpv"].tolist()))
                wph |= set(zip(ph["wph"].tolist(), ph["wpv"].tolist()))
            b = bands(a)
            assert (b[:, 0] != 0).all()
            y0r |= set((a["y0"] & 3).tolist())
            y1r |= set((a["y1"] & 3).tolist())
            in_area = (a["t4y"] >= a["y0"]) & (a["t4y"] <= a["y1"]) & (a["t4x"] >= a["x0"]) & (a["t4x"] <= a["x1"])
            t4_in += int(in_area.sum())
            t4_skipped += int((((b[:, 0] >> (a["t4y"] >> 2)) & 1) == 0).sum())
            wave1_off += int((b[:, 1] == 0).sum())
            origins |= set(a["tx"].tolist())
        assert y0r == {0, 1, 2, 3} and y1r == {0, 1, 2, 3}, (ocw, y0r, y1r)       # every band boundary is a skip edge
        assert t4_in >= 4 and t4_skipped >= 4 and wave1_off >= 4, (ocw, t4_in, t4_skipped, wave1_off)
        assert len(origins) >= 2                                                 # tiles at origin 1 and centred tiles
        assert len(cph) == 16 and {p[0] for p in wph} == {0, 1, 2, 3} and len({p[1] for p in wph}) >= 2, (ocw, len(cph), wph)


@pytest.mark.parametrize("ocw", OCWS)
def test_climbs_stay_inside_the_area(oracle, ocw):
    """the fixtures are chosen so that the climbs stay inside the area: at least 90 % of the clean points of every ordinary fixture, by
    the speculative climb restated in numpy -- whose surface is the oracle's (its peak value is the oracle's, bit for bit)"""
    for sx, sy in DIRECTIONS:
        for o in RESTATED[ocw]:
            inside = ordinary_inside(ocw, sx, sy, o)
            print(ocw, (sx, sy), o, "points whose climbs stay inside:", int(inside.sum()), "of", inside.size)
            assert inside.mean() >= 0.9, (ocw, sx, sy, o, inside)
        case = direction_case(ocw, sx, sy)
        want = oracle.match(*case)
        best = np.array([max(val[cy, cx] for centres, _, _ in speculative_climbs(case, g, val) for cx, cy in centres)
                         for g in range(4) for val in (surface(case, g),)], np.float32)
        assert_bits_equal(best, want[:4, 2], f"peak values ocw {ocw} {(sx, sy)}")


def test_rounding_targets_lie_inside_the_area():
    """the ambiguous cell of every clean point of the rounding-boundary fixtures lies inside the point's area: its band is finished, and
    the redo pass runs on it while other bands are skipped"""
    for ocw in OCWS:
        case = edge_case(ocw)
        a = areas(case)
        t = case[7]
        clean = np.flatnonzero(a["clean"])
        assert clean.size >= 8
        skipping = 0
        for g in clean:
            assert t[g, ec.T_FORM] == 0
            lu, lv = a["last"][g]
            rx = abs(lu) + 2 + int(t[g, ec.T_SU]) - a["tx"][g]                    # pivot (0, 0)'s cell is dx2 - ocw = |lu| + 2
            ry = abs(lv) + 2 + int(t[g, ec.T_SV]) - a["ty"][g]
            assert a["x0"][g] <= rx <= a["x1"][g] and a["y0"][g] <= ry <= a["y1"][g], (ocw, g)
            skipping += int(bands(a)[g].tolist() != [255, 255])
        print(ocw, "clean points", clean.size, "of which with skipped bands", skipping)
        assert skipping >= 1


def test_c2_areas_of_the_clean_points():
    """BASELINE C2 on record: the classes are unchanged (96,939 clean, 17,814 on the advance list), and the clean points' areas meet 5 or 6
    of the 8 row bands and both column halves"""
    from mimc3_amd import api
    c = synth.make_case("C2")
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, 16, *c.i0.shape)
    a = areas((c.i0, c.i1, c.xyuvav, c.offset, off, uv, 16))
    assert int(a["clean"].sum()) == 96939 and int(a["advance"].sum()) == 17814
    b = bands(a)[a["clean"]]
    nb = np.array([bin(int(v)).count("1") for v in np.unique(b[:, 0])])
    print("C2 clean points: bands per wave-0 mask", sorted(set(nb.tolist())), "wave 1 idle:", int((b[:, 1] == 0).sum()))
    assert set(nb.tolist()) <= {5, 6} and (b[:, 1] == b[:, 0]).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def match_both_ways(ctx, oracle, case, what):
    i0, i1, xy, offset, off, uv, ocw = case[:7]
    offset = np.asarray(offset, np.int32)
    got = ctx.matching_ncc_dlc_2(xy, offset, off, uv, ocw)
    assert ctx.last_path() == "u8_mfma", what
    assert_bits_equal(got, oracle.match(i0, i1, xy, offset, off, uv, ocw), f"{what}: auto vs oracle")
    sw = ctx.matching_ncc_dlc_2(xy, -offset, off, -uv, ocw, swap=True)
    assert_bits_equal(sw, oracle.match(i1, i0, xy, -offset, off, -uv, ocw), f"{what} swapped: auto vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_directions_lengths_and_phases(api, oracle, ocw):
    """every direction, every corridor length, every pixel phase: the oracle's bits; the matrix-core launch finishes exactly the clean
    points whose speculative climbs stay inside the area (at least 90 % of them), the others are appended to the rest list"""
    cases = [(sx, sy, o) for sx, sy in DIRECTIONS for o in OFFSETS]
    with api.Context(0) as ctx:
        for sx, sy, o in cases:
            case = direction_case(ocw, sx, sy, o)
            ctx.set_images(case[0], case[1])
            match_both_ways(ctx, oracle, case, f"ocw {ocw} direction {(sx, sy)} offset {o}")
    stats = ac.advance_stats("import test_mx_area_finish as t; cases = [t.direction_case(%d, sx, sy, o) for sx, sy, o in %r]" % (ocw, cases))
    assert len(stats) == len(cases)
    for (sx, sy, o), (l_clean, l_rest, done, rest_after, n_adv, tried, fin) in zip(cases, stats):
        print(ocw, (sx, sy), o, "clean list", l_clean, "finished", done, "rest list", l_rest, "->", rest_after)
        assert (l_clean, l_rest, n_adv) == (20, 0, 0)
        assert l_clean - done == rest_after - l_rest and done >= 0.9 * l_clean
        if o in RESTATED[ocw]:
            assert done == int(ordinary_inside(ocw, sx, sy, o).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_rounding_boundaries_under_skipping(api, oracle, ocw):
    """the rounding-boundary fixtures: the redo path on cells inside the area; every clean point is finished by the matrix-core launch"""
    case = edge_case(ocw)
    with api.Context(0) as ctx:
        ctx.set_images(case[0], case[1])
        match_both_ways(ctx, oracle, case, f"rounding ocw {ocw}")
    (st,) = ac.advance_stats("import test_mx_area_finish as t; cases = [t.edge_case(%d)[:7]]" % ocw)
    print("rounding", ocw, st)
    assert st[0] == int(areas(case)["clean"].sum()) and st[2] >= 0.9 * st[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_clean_points_that_leave_their_area(api, oracle, ocw):
    """a shift far off the corridor, no nulls: clean points leave their area, are handed on and finished by the register-tiled launch
    with the oracle's bits; the rest list grows by exactly the points the restated climb sends there"""
    case = off_corridor_case(api, ocw)
    a = areas(case)
    clean = np.flatnonzero(a["clean"])
    leave = [g for g in clean if not stays_inside(case, a, g)]
    assert len(leave) >= 3 and a["advance"].sum() == 0
    with api.Context(0) as ctx:
        ctx.set_images(case[0], case[1])
        match_both_ways(ctx, oracle, case, f"off-corridor ocw {ocw}")
    (st,) = ac.advance_stats("import test_mx_area_finish as t; cases = [t.off_corridor_case(api, %d)]" % ocw)
    l_clean, l_rest, done, rest_after = st[:4]
    print("off-corridor", ocw, "clean list", l_clean, "finished", done, "rest list", l_rest, "->", rest_after, "numpy: leave", len(leave))
    assert l_clean == clean.size and l_rest == int((~a["clean"]).sum())
    assert l_clean - done == rest_after - l_rest == len(leave)


@pytest.mark.gpu
def test_switches(api, tmp_path):
    """MIMC3_MX_AREA=0, MIMC3_U8_RECS=0, MIMC3_U8_ADVANCE=0: the same bytes; without areas only a climb that leaves the tile is handed on"""
    body = ("import test_mx_area_finish as t; cases = [t.direction_case(16, 1, -1), t.direction_case(7, -1, 1, (3, 1)), "
            "t.off_corridor_case(api, 16), t.edge_case(16)[:7], ac.blobs_case(api, 16)]")
    on = ac.advance_stats(body, outdir=str(tmp_path / "on"))
    assert len(on) == 5
    for name, env in (("area_off", {"MIMC3_MX_AREA": "0"}), ("records_off", {"MIMC3_U8_RECS": "0"}), ("advance_off", {"MIMC3_U8_ADVANCE": "0"})):
        off_ = ac.advance_stats(body, env=env, outdir=str(tmp_path / name))
        print(name, off_)
        assert [s[:2] for s in off_] == [s[:2] for s in on], name                 # the classifier's lists do not depend on the switches
        assert all(s[0] - s[2] <= t[0] - t[2] for s, t in zip(off_, on)), name     # whole-tile areas: no more hand-ons than with areas
        for i in range(5):
            assert_bits_equal(np.load(tmp_path / name / f"{i}.npy"), np.load(tmp_path / "on" / f"{i}.npy"), f"{name} call {i}")
    assert on[2][0] - on[2][2] > 0
