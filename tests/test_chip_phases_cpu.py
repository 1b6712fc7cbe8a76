"""CPU: the fixtures of tests/chip_phase_common.py qualified, over exactly the calls tests/test_chip_phases.py and
tests/test_chip_phases_acc.py make.

  * every case of section 1 reaches every (chip phase, window phase, null class) cell -- a condition on the fixture: if it does not hold,
    change the fixture, never the condition; its points are live, and a chip or window read one pixel aside changes every surface;
  * every case of section 2 holds exactly one null per point, where the list says, and moving that null by one pixel changes the surface;
    the wide kernel's per-tile null query, restated, finds each planted null in exactly the tile windows the intervals say;
    on the u16 planes every tile of the grid has a null in the first and last column and row of its window and one a pixel outside;
  * the comparison the GPU tests use rejects an oracle surface whose chip was read one pixel aside, and one with a null left unmasked;
  * the judge of the accumulating forms (chip_phase_common.acc_judge) takes NumpyStack fed the oracle's layer, and rejects a stack into
    which the layer went twice -- as a layer, or cell by cell behind one layer count -- and a layer whose chip was read one pixel aside."""
import numpy as np
import pytest

import chip_phase_common as cp
from phase_common import fractional, plane_end_points, search_shifts, trunc
from stack_common import NumpyStack, refused_of
from u8_advance_common import BORDER

PHASE_IDS = [cp.case_id(c) for c in cp.PHASE_CASES]
SWEEP_IDS = [cp.case_id(c) for c in cp.SWEEP_CASES]


# ---- 1. the coverage condition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cp.PHASE_CASES, ids=PHASE_IDS)
def test_every_phase_pair_occurs_with_every_null_class(case):
    """over the forward calls of the GPU test's own list (the two swapped calls add cells, none is needed).  On the u16 planes the kernel's
    cells are the `& 1` parities times the null class; the `& 3` cells are asserted there too"""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    assert len(calls) == 10 and sum(1 for c in calls if c[2]) == 2
    cells = cp.call_cells(f, radius, [c for c in calls if not c[2]])
    assert all(cells[(a, b, null)] >= 1 for a in range(4) for b in range(4) for null in range(4)), \
        [k for k in ((a, b, null) for a in range(4) for b in range(4) for null in range(4)) if cells[k] < 1]
    if entry in ("planes", "wplanes"):
        par = {(a & 1, b & 1, null) for (a, b, null), n in cells.items() if n}
        assert len(par) == 16
    sw = cp.call_cells(f, radius, [c for c in calls if c[2]])
    assert len({k[:2] for k in sw}) >= 8                        # (the swapped calls: at least two of the four window phases)


def test_the_gpu_tests_parts_make_every_call_of_every_case_once():
    """a case in halves (chip_phase_common.HALVES) makes the ten calls that the parts of PARTS make: the conditions below, which run
    over PARTS, are conditions on the GPU test's own calls"""
    for case in cp.PHASE_CASES:
        made = sorted(k for c, p in cp.PHASE_PARTS if c == case for k in cp.part_calls(p))
        assert made == list(range(10)) == sorted(k for p in cp.PARTS for k in cp.PARTS[p]), case
    assert len(cp.PHASE_PARTS) == 3 * len(cp.PHASE_CASES) + 2 * len(cp.HALVED_CASES) and set(cp.HALVED_CASES) <= set(cp.PHASE_CASES)


def test_the_grids_beyond_16_px_keep_odd_spacings_and_boxes_apart():
    from phase_common import LU_MAX, LV_MAX, geometry
    for _, _, ocw, radius in cp.PHASE_CASES:
        if radius <= 16:
            continue
        H, W, mu, mv, su, sv = geometry(ocw, radius)
        assert su % 2 == 1 and sv % 2 == 1
        side = 2 * (radius + ocw) + 1
        assert su >= side + 2 * (LU_MAX + 3) and sv >= side + 2 * (LV_MAX + 3)            # boxes apart under every shift and offset
        assert mu - (radius + ocw + LU_MAX + 3) >= 0 and mv - (radius + ocw + LV_MAX + 3) >= 0      # and inside the image
        assert H <= 1300 and W <= 1300


def test_an_eighths_pair_holds_the_integers_of_the_12_bit_pair():
    for ocw in (1, 10, 57):
        a, b = cp.phase_fixture(("planes", "12bit", ocw, 7)), cp.phase_fixture(("planes", "eighths", ocw, 7))
        for x, y in zip(cp.integer_images(a), cp.integer_images(b)):
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(a.xy, b.xy) and not np.array_equal(a.i0, b.i0)


@pytest.mark.parametrize("part", list(cp.PARTS))
@pytest.mark.parametrize("case", [c for c in cp.PHASE_CASES if c[1] != "eighths"], ids=[i for i, c in zip(PHASE_IDS, cp.PHASE_CASES) if c[1] != "eighths"])
def test_points_are_live_in_every_call(case, part):
    """At least 48 of the 64 points have a finite oracle surface and a status >= -1 in every call.  (An eighths case reads the oracle of
    its 12-bit case.)  At R 1 the surface has one cell that is no border cell, so a point is finished only where the true displacement IS
    the search centre -- which no pair can give at four offsets: there every maximum lies on the border (status -4), and the condition
    is a finite surface and a status other than -2 and -3.
    At ocw 10 and 57: the chip image or the window image rolled by one pixel changes the surface of every valid point, so a staging that
    is one phase off cannot pass."""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    for k in cp.PARTS[part]:
        (rec, surf), (offset, shift, swap) = cp.phase_oracle(case, k), calls[k]
        fin = np.isfinite(surf).all(axis=1)
        live = fin & ((rec[:, 2] >= -1) if radius > 1 else ((rec[:, 2] != -2) & (rec[:, 2] != -3)))
        assert live.sum() >= 48, (offset.tolist(), shift is not None, swap, int(live.sum()))
    if ocw in (10, 57) and part == "prior":
        k = 2                                                   # offset (1, 0) with the a-priori shift
        rec, surf = cp.phase_oracle(case, k)
        valid = np.isfinite(surf).all(axis=1) & (rec[:, 2] >= -1)
        q0, q1 = cp.integer_images(f)
        for images, what in (((np.roll(q0, 1, axis=1), q1), "chip"), ((q0, np.roll(q1, 1, axis=1)), "window")):
            other = cp.oracle_search(f, radius, *calls[k], images=images)[1]
            same = (np.nan_to_num(other).view(np.uint32) == np.nan_to_num(surf).view(np.uint32)).all(axis=1)
            assert not (same & valid).any(), f"{what} moved by one pixel: points {np.flatnonzero(same & valid).tolist()} keep their surface"


# ---- 2. one null per point ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cp.SWEEP_CASES, ids=SWEEP_IDS)
def test_every_point_holds_exactly_its_planted_null(case):
    entry, kind, ocw, radius = case
    fx = cp.sweep_fixture(case)
    cw = 2 * ocw + 1
    d2 = cw + 2 * radius
    nc, nb = cp.null_counts(fx)
    chip = np.array([s == "chip" for s, _, _ in fx.nulls])
    assert np.array_equal(nc, chip.astype(int)) and np.array_equal(nb, (~chip).astype(int))
    assert int((fx.i0 == 0).sum()) == chip.sum() and int((fx.i1 == 0).sum()) == (~chip).sum() and (fx.b0 > 0).all() and (fx.b1 > 0).all()
    for k, (side, x, y) in enumerate(fx.nulls):                 # ... where the list says
        img, px, py = (fx.i0, fx.cu[k] + x, fx.cv[k] + y) if side == "chip" else (fx.i1, fx.wu[k] + x, fx.wv[k] + y)
        assert img[py, px] == 0 and 0 <= x < (cw if side == "chip" else d2) and 0 <= y < (cw if side == "chip" else d2)
    # the list holds what the positions are for
    ccols = {x for s, x, _ in fx.nulls if s == "chip"}
    assert ccols == {c for c in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, cw - 2, cw - 1) if 0 <= c < cw}
    assert {y for s, _, y in fx.nulls if s == "chip"} <= {0, 1, ocw, cw - 1}
    bcols, brows = {x for s, x, _ in fx.nulls if s == "box"}, {y for s, _, y in fx.nulls if s == "box"}
    assert bcols >= {c for c in (0, 1, 2, 3, 15, 16, 63, 64, 79, 80, d2 - 2, d2 - 1) if 0 <= c < d2}
    assert brows >= {r for r in (0, 15, 16, 63, 64, 127, 128, d2 - 1) if 0 <= r < d2}
    if ocw >= 2:
        assert {x & 3 for x in ccols} == {0, 1, 2, 3} and {x & 3 for x in bcols} == {0, 1, 2, 3}       # every byte lane of a dword
    assert len({(int(a) & 3, int(b) & 3) for a, b in zip(fx.cu, fx.wu)}) >= 8                          # and the phases vary under them
    # every search box inside the image, no two overlapping
    H, W = fx.i0.shape
    assert fx.wu.min() >= 0 and fx.wv.min() >= 0 and (fx.wu + d2).max() <= W and (fx.wv + d2).max() <= H
    n = len(fx.nulls)
    for a in range(n):
        for b in range(a + 1, n):
            assert abs(int(fx.wu[a] - fx.wu[b])) >= d2 + 2 or abs(int(fx.wv[a] - fx.wv[b])) >= d2 + 2


@pytest.mark.parametrize("case", cp.SWEEP_CASES, ids=SWEEP_IDS)
def test_a_null_moved_by_one_pixel_changes_the_surface(case):
    """otherwise the case could not tell a mask that is one byte off from the right one"""
    fx = cp.sweep_fixture(case)
    rec, surf = cp.sweep_oracle(fx)
    assert (np.isfinite(surf).all(axis=1) & (rec[:, 2] >= -1)).all()
    base = cp.sweep_oracle(fx, images=(fx.b0, fx.b1))[1]
    moved = cp.sweep_oracle(fx, images=cp.sweep_moved(fx))[1]
    for k, null in enumerate(fx.nulls):
        assert (surf[k].view(np.uint32) != moved[k].view(np.uint32)).any(), (k, null)
        assert (surf[k].view(np.uint32) != base[k].view(np.uint32)).any(), (k, null)        # and the null shows at all


@pytest.mark.parametrize("case", [c for c in cp.SWEEP_CASES if c[0] in cp.WIDE], ids=[i for i, c in zip(SWEEP_IDS, cp.SWEEP_CASES) if c[0] in cp.WIDE])
def test_the_tile_query_finds_each_null_in_exactly_its_tile_windows(case):
    entry, kind, ocw, radius = case
    fx = cp.sweep_fixture(case)
    cw, S = 2 * ocw + 1, 2 * radius + 1
    win = cp.tile_windows(ocw, radius)
    nt = (S + 31) // 32
    assert len(win) == nt and win[0][0] == 0 and win[-1][1] == cw + 2 * radius - 1          # the windows cover the box, end to end
    seen = cp.wn_tiles_of_every_point(fx)
    for (side, x, y), tiles in zip(fx.nulls, seen):
        assert tiles == (set() if side == "chip" else cp.tiles_holding(x, y, ocw, radius)), (side, x, y, tiles)
    # the four positions per tile and axis are in the list, and lie on the side of the window's edge they are meant for
    box = {(x, y) for s, x, y in fx.nulls if s == "box"}
    for t, (a, b) in enumerate(win):
        for axis in (0, 1):
            for c, inside in ((a - 1, False), (a, True), (b, True), (b + 1, False)):
                if not 0 <= c < cw + 2 * radius:
                    continue
                pts = [p for p in box if p[axis] == c]
                assert pts, (t, axis, c)
                for p in pts:
                    assert (t in {tile[axis] for tile in cp.tiles_holding(p[0], p[1], ocw, radius)}) == inside, (t, axis, c, p)
    assert any(len(t) == 1 for t in seen) and any(len(t) >= 2 for t in seen)
    if entry != "wplanes":
        return
    # every tile of the grid, on each axis: a point whose null sits IN the first | last column (row) of the tile's window, and the query
    # of that tile sees it; a point whose null sits one pixel OUTSIDE it (where the box has that pixel), and the query does not
    point = {(x, y): k for k, (s, x, y) in enumerate(fx.nulls) if s == "box"}
    met = set()
    for tx, ty, axis, inside, (x, y) in cp.tile_edge_nulls(ocw, radius):
        a, b = win[(tx, ty)[axis]]
        c, d = win[(ty, tx)[axis]]
        edge = (x, y)[axis]
        assert edge in ((a, b) if inside else (a - 1, b + 1)) and c <= (x, y)[1 - axis] <= d, (tx, ty, axis, inside, x, y)
        assert ((tx, ty) in seen[point[(x, y)]]) == inside, (tx, ty, axis, inside, x, y)
        met.add((tx, ty, axis, edge - a if edge <= a else edge - b + 2))
    for ty in range(nt):
        for tx in range(nt):
            for axis in (0, 1):
                a, b = win[(tx, ty)[axis]]
                want = {0, 2} | ({-1} if a > 0 else set()) | ({3} if b + 1 < cw + 2 * radius else set())
                assert {m[3] for m in met if m[:3] == (tx, ty, axis)} == want, (tx, ty, axis)


# ---- 3. plane ends, fractions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cp.PLANE_END_CASES, ids=[cp.case_id(c) for c in cp.PLANE_END_CASES])
def test_plane_end_points_end_in_the_last_row_and_column_and_are_refused(case):
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    exy, eshift = plane_end_points(f, radius)
    H, W = f.i0.shape
    u0, v0 = trunc(exy)
    assert int(v0[0] + eshift[0, 1]) + radius + ocw == H + BORDER - 1 and int(u0[1] + eshift[1, 0]) + 3 + radius + ocw == W + BORDER - 1
    for offset in cp.U_OFFSETS:
        rec, surf = cp.oracle_search(f, radius, np.asarray(offset, np.int32), eshift, False, xy=exy)
        assert (rec[:, 2] == -3).all() and np.isnan(surf).all()


def test_the_fractional_grids_truncate_to_the_fixture():
    for case in cp.FRACTIONAL_CASES:
        f = cp.phase_fixture(case)
        for seed in (5, 6):
            fr = fractional(f.xy, seed)
            assert np.array_equal(trunc(fr)[0], trunc(f.xy)[0]) and np.array_equal(trunc(fr)[1], trunc(f.xy)[1]) and not np.array_equal(fr, f.xy)
    f = cp.phase_fixture(cp.FRACTIONAL_CASES[0])
    prior = search_shifts(f)[0]
    a = cp.oracle_search(f, 7, cp.FR_OFFSET, prior, False, xy=fractional(f.xy, 5))
    b = cp.oracle_search(f, 7, cp.FR_OFFSET, prior, False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- the comparison rejects a plausible error -------------------------------------------------------------------------------------------------
def as_a_kernel_would_return(surf, rec, shift, radius, npeaks):
    """a consistent result around a given surface: record and candidates are its own tail"""
    from full_any_common import tail_from_surface
    t_rec, t_cand = tail_from_surface(surf, shift, radius, npeaks, refused=rec[:, 2] == -3, device_snr_order=True)
    return t_rec, t_cand, surf


@pytest.mark.parametrize("case", [("class", "u8", 10, 7), ("planes", "12bit", 57, 7), ("wide", "u8", 7, 32), ("wplanes", "12bit", 7, 32)], ids=cp.case_id)
def test_the_comparison_rejects_a_chip_read_one_pixel_aside(case):
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    q0, q1 = cp.integer_images(f)
    for k in (2, 8):                                            # forward and swapped
        offset, shift, swap = calls[k]
        o_rec, o_surf = cp.phase_oracle(case, k)
        for npeaks in cp.NPEAKS:
            cp.vs_oracle(as_a_kernel_would_return(o_surf, o_rec, shift, radius, npeaks), o_rec, o_surf, shift, radius, npeaks, "the oracle itself")
        aside = (q0, np.roll(q1, 1, axis=1)) if swap else (np.roll(q0, 1, axis=1), q1)
        p_rec, p_surf = cp.oracle_search(f, radius, offset, shift, swap, images=aside)
        with pytest.raises(AssertionError):
            cp.vs_oracle(as_a_kernel_would_return(p_surf, p_rec, shift, radius, 4), o_rec, o_surf, shift, radius, 4, "chip one pixel aside")


@pytest.mark.parametrize("case", [("class", "u8", 10, 7), ("planes", "spread12", 57, 7), ("wide", "u8", 25, 32), ("wplanes", "spread12", 25, 32)], ids=cp.case_id)
def test_the_comparison_rejects_one_null_left_unmasked(case):
    """one planted null read as a pixel (of 1, the darkest there is) and not masked: one point's surface differs, and the comparison of
    the whole launch fails -- for the first chip null (column 0), the last (CW - 1), and the last box null"""
    fx = cp.sweep_fixture(case)
    o_rec, o_surf = cp.sweep_oracle(fx)
    cp.vs_oracle(as_a_kernel_would_return(o_surf, o_rec, fx.shift, fx.R, 4), o_rec, o_surf, fx.shift, fx.R, 4, "the oracle itself")
    last_chip = max(k for k, n in enumerate(fx.nulls) if n[0] == "chip")
    for k in (0, last_chip, len(fx.nulls) - 1):
        side, x, y = fx.nulls[k]
        i0, i1 = fx.i0.copy(), fx.i1.copy()
        if side == "chip":
            i0[fx.cv[k] + y, fx.cu[k] + x] = 1
        else:
            i1[fx.wv[k] + y, fx.wu[k] + x] = 1
        p_rec, p_surf = cp.sweep_oracle(fx, images=(i0, i1))
        differs = [(p_surf[g].view(np.uint32) != o_surf[g].view(np.uint32)).any() for g in range(len(fx.nulls))]
        assert differs[k] and sum(differs) == 1
        with pytest.raises(AssertionError):
            cp.vs_oracle(as_a_kernel_would_return(p_surf, p_rec, fx.shift, fx.R, 4), o_rec, o_surf, fx.shift, fx.R, 4, "a null left unmasked")


# ---- the judge of the accumulating forms ------------------------------------------------------------------------------------------------------
def finishes_of(stack):
    return [stack.finish(k, mc) for k, mc in cp.ACC_FINISHES]


def test_the_accumulating_cases_are_search_cases_and_reach_every_instantiation():
    """every ACC case is a case of the search lists (it reads that case's oracle); per entry KCW = (CW + 15 + 63) / 64, the K chunks per
    chip row and 16 x 16 cell tile that the kernels are instantiated on, is 1, 2 and 3"""
    assert set(cp.ACC_PHASE_CASES) <= set(cp.PHASE_CASES) and set(cp.ACC_SWEEP_CASES) <= set(cp.SWEEP_CASES)
    assert set(cp.ACC_PARTS) <= set(cp.PARTS)
    for entry in cp.ENTRIES:
        assert sorted((2 * c[2] + 1 + 15 + 63) // 64 for c in cp.ACC_PHASE_CASES if c[0] == entry) == [1, 2, 3]
        assert sum(1 for c in cp.ACC_SWEEP_CASES if c[0] == entry) == 1


@pytest.mark.parametrize("part", cp.ACC_PARTS)
@pytest.mark.parametrize("case", cp.ACC_PHASE_CASES, ids=[cp.case_id(c) for c in cp.ACC_PHASE_CASES])
def test_one_oracle_layer_in_numpy_stack_is_what_the_acc_judge_takes(case, part):
    """NumpyStack fed the oracle's surface and refused_of(its record): the mean at (4, 1) is that surface at finite cells and NaN
    elsewhere, one layer per point that is not refused, all NaN at (0, 2) -- and the judge takes it.  Every call holds points of the clean
    form (no null in chip or box) and of the masked form"""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    for k in cp.PARTS[part]:
        offset, shift, swap = calls[k]
        o_rec, o_surf = cp.phase_oracle(case, k)
        stack = NumpyStack(f.xy.shape[0], radius, shift).add(o_surf, refused_of(o_rec))
        (rec, cand, lay, mean), (rec2, cand2, lay2, mean2) = finishes_of(stack)
        fin = np.isfinite(o_surf)
        assert np.array_equal(mean.view(np.uint32)[fin], o_surf.view(np.uint32)[fin]) and np.isnan(mean[~fin]).all()
        assert np.array_equal(lay, (o_rec[:, 2] != -3).astype(np.uint16)) and np.isnan(mean2).all() and (lay == 1).sum() >= 48
        cp.acc_judge(finishes_of(stack), o_rec, o_surf, radius, shift, "NumpyStack over the oracle's layer")
        null = cp.call_cells(f, radius, [calls[k]])
        # (one point of each is what it takes to launch both forms; four of 64 is more than an accident of the grid)
        assert sum(n for c, n in null.items() if c[2] == 0) >= 4 and sum(n for c, n in null.items() if c[2] != 0) >= 4


@pytest.mark.parametrize("case", cp.ACC_SWEEP_CASES, ids=[cp.case_id(c) for c in cp.ACC_SWEEP_CASES])
def test_every_sweep_point_is_the_masked_forms_and_the_acc_judge_takes_the_oracle(case):
    fx = cp.sweep_fixture(case)
    nc, nb = cp.null_counts(fx)
    assert ((nc > 0) | (nb > 0)).all()
    o_rec, o_surf = cp.sweep_oracle(fx)
    stack = NumpyStack(len(fx.nulls), fx.R, fx.shift).add(o_surf, refused_of(o_rec))
    assert (stack.lay == 1).all()
    cp.acc_judge(finishes_of(stack), o_rec, o_surf, fx.R, fx.shift, "NumpyStack over the oracle's layer")


@pytest.mark.parametrize("case", [("class", "u8", 10, 7), ("planes", "12bit", 57, 7), ("wide", "u8", 10, 16), ("wplanes", "12bit", 25, 32)], ids=cp.case_id)
def test_the_acc_judge_rejects_a_layer_added_twice_and_a_chip_read_one_pixel_aside(case):
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    n = f.xy.shape[0]
    q0, q1 = cp.integer_images(f)
    for k in (2, 8):                                            # forward and swapped
        offset, shift, swap = calls[k]
        o_rec, o_surf = cp.phase_oracle(case, k)
        refused = refused_of(o_rec)
        twice = NumpyStack(n, radius, shift).add(o_surf, refused).add(o_surf, refused)
        with pytest.raises(AssertionError):
            cp.acc_judge(finishes_of(twice), o_rec, o_surf, radius, shift, "the layer twice")
        # the cells twice behind ONE layer count -- what a point finished by the clean AND the masked launch would leave: the mean at
        # (4, 1), the counts, record and candidates are the right ones, and only min_count 2 shows it
        cells = NumpyStack(n, radius, shift).add(o_surf, refused).add(o_surf, np.ones(n, bool))
        right = finishes_of(NumpyStack(n, radius, shift).add(o_surf, refused))
        for a, b in zip(finishes_of(cells)[0], right[0]):
            assert a.tobytes() == b.tobytes()
        with pytest.raises(AssertionError, match="min_count 2"):
            cp.acc_judge(finishes_of(cells), o_rec, o_surf, radius, shift, "the cells twice")
        one = np.zeros(n, bool)
        one[int(np.flatnonzero(~refused)[5])] = True                # ... and of ONE point only
        s1 = np.where(one[:, None], o_surf, np.float32(np.nan))
        cells = NumpyStack(n, radius, shift).add(o_surf, refused).add(s1, np.ones(n, bool))
        with pytest.raises(AssertionError, match="min_count 2"):
            cp.acc_judge(finishes_of(cells), o_rec, o_surf, radius, shift, "one point's cells twice")
        aside = (q0, np.roll(q1, 1, axis=1)) if swap else (np.roll(q0, 1, axis=1), q1)
        p_rec, p_surf = cp.oracle_search(f, radius, offset, shift, swap, images=aside)
        with pytest.raises(AssertionError):
            cp.acc_judge(finishes_of(NumpyStack(n, radius, shift).add(p_surf, refused_of(p_rec))), o_rec, o_surf, radius, shift, "chip one pixel aside")
