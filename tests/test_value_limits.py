"""GPU: every integer matcher at the top of its pixel class, bit for bit against the CPU oracles.

The integer kernels are exact because their sums fit the fields and lanes they are kept in; the fixtures of tests/value_limit_common.py
(qualified on the CPU by tests/test_value_limits_cpu.py) hold chips that sum to 99 % and more of a chip of `top` pixels -- the most the
fields of sat_kernel.h and the lanes of match_px_kernel.hip, match_mx_kernel.hip, match_full_u16_kernel.hip and match_full_f32_kernel.hip
can be asked to hold (that is about 0.80 of 2^21, 2^25 and 2^33: the fields are sized for it, and fail one bit narrower).

  * the DLC matcher (matching_ncc_dlc_2 against oracle.match) in every path mode, forward and swapped, last_path asserted;
  * the exhaustive search (match_ncc_full, _full_multi, _full_planes, _full_dn, and _full_any(mode=1) on one config per class) against
    the class's oracle at npeaks 8 -- on 8-bit pairs also with whole search boxes on either side of the 8,224 pixels up to which one
    packed table query counts nulls exactly;
  * one null pixel in an otherwise null-free pair at the top of the 8-bit class: a null count read as 0 cannot pass;
  * the classifier's statistic on null-free pairs whose windows exceed 8,224 pixels: every point clean (what a forgotten split changes);
  * class edges: one pixel one above the top moves the pair to the next class, and the result still equals the oracle's.

Refusals: tests/test_search_refusals.py pins that match_ncc_full_planes refuses a 16-bit pair and match_ncc_full_dn a float pair, on
pairs far inside those classes; the pairs exactly one above the top (4096, 2^20) are pinned here."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_search_common import assert_records_match, full_search
from value_limit_common import (CLASSES, DLC_CASES, DLC_NULL_ANGLE, DLC_NULL_OCW, DLC_NULL_SPEED, FULL_CASES, FULL_R, MODES,
                                PACKED_QUERY_PIXELS, base_pair, case_id, class_pair, dlc_windows, exhaustive_oracle,
                                expected_path_at_limits, grid_uv, one_null)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.fixture(autouse=True)
def records_as_shipped(monkeypatch):
    monkeypatch.delenv("MIMC3_U8_RECS", raising=False)


# ---- the DLC matcher -------------------------------------------------------------------------------------------------------------------
def dlc_both_ways(api, oracle, ctx, i0, i1, c, ocw, what, modes=MODES, paths=None):
    """every path mode, forward and swapped, against oracle.match; -> the paths taken, by mode"""
    H, W = i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    want = oracle.match(i0, i1, c.xyuvav, c.offset, off, uv, ocw)
    want_sw = oracle.match(i1, i0, c.xyuvav, -c.offset, off, -uv, ocw)
    taken = {}
    for mode in modes:
        ctx.set_path(mode)
        got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, ocw)
        taken[mode] = ctx.last_path()
        sw = ctx.matching_ncc_dlc_2(c.xyuvav, -c.offset, off, -uv, ocw, swap=True)
        assert ctx.last_path() == taken[mode], f"{what}, mode {mode}: the swapped call took {ctx.last_path()}"
        expect = (paths or {}).get(mode) or expected_path_at_limits(mode, i0, i1, ocw)
        assert taken[mode] == expect, f"{what}, mode {mode}: {taken[mode]}, expected {expect}"
        assert_bits_equal(got, want, f"{what}, mode {mode} ({taken[mode]})")
        assert_bits_equal(sw, want_sw, f"{what}, mode {mode} ({taken[mode]}), swapped")
    ctx.set_path("auto")
    return taken


@pytest.mark.parametrize("case", DLC_CASES, ids=case_id)
def test_dlc_matcher_at_the_top_of_the_class(api, oracle, case):
    kind, spread, ocw, null_frac = case
    c, i0, i1 = class_pair(*case)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        taken = dlc_both_ways(api, oracle, ctx, i0, i1, c, ocw, case_id(case))
    print(case_id(case), taken)
    if kind == "u8":
        assert taken["auto"] == "u8_mfma" and taken["u8px"] == "u8_exact" and taken["u16"] == "u16_scaled"
    elif kind == "9bit" and spread == 254:
        assert taken["auto"] == "u8_offset"             # a global range of 254: every chip and window fits the offset scheme
    elif kind == "9bit":
        assert taken["auto"] in ("u8_offset", "u16_scaled")            # (a range of 255 in every 128 x 128 tile: the scheme is not tried)
    elif kind == "9bit_local":
        assert taken["auto"] == "u8_offset"             # tried, and the points that overflow by one come back through the u16 list
    elif kind == "12bit":
        assert taken["auto"] == "u8_offset" and taken["u16"] == "u16_scaled"       # spread <= 63: PxU8o with offsets near 4095 - 255
    elif kind in ("eighths", "mixed"):
        assert taken["auto"] == "u16_scaled"
    else:
        assert taken["auto"] == "f32_tiled" and taken["general"] == "general_f32"


# ---- the exhaustive search ---------------------------------------------------------------------------------------------------------------
def search_both_ways(api, ctx, kind, i0, i1, c, ocw, radius, what, any_mode1=False):
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    path = CLASSES[kind][5]
    for swap in (False, True):
        sgn = -1 if swap else 1
        off, sh = sgn * c.offset, sgn * shift
        w = f"{what}, swap {swap}"
        want_rec, want = exhaustive_oracle(kind, i0, i1, c.xyuvav, off, ocw, radius, sh, swap)
        if kind == "u8":
            rec = ctx.match_ncc_full(c.xyuvav, off, ocw, radius, shift=sh, swap=swap)
            assert ctx.last_path() == path
            assert_records_match(rec, full_search(i0, i1, c.xyuvav, off, ocw, radius, shift=sh, swap=swap), w + ": match_ncc_full")
            out, cand = ctx.match_ncc_full_multi(c.xyuvav, off, ocw, radius, 8, shift=sh, swap=swap)
            assert ctx.last_path() == path
            assert_bits_equal(out, rec, w + ": match_ncc_full_multi's record vs match_ncc_full's")
        elif CLASSES[kind][4] == "u16":
            out, cand = ctx.match_ncc_full_planes(c.xyuvav, off, ocw, radius, 8, shift=sh, swap=swap)
            assert ctx.last_path() == path
        else:
            out, cand = ctx.match_ncc_full_dn(c.xyuvav, off, ocw, radius, 8, shift=sh, swap=swap)
            assert ctx.last_path() == path
        assert_records_match(out, want_rec, w + ": record")
        assert_bits_equal(cand, want, w + ": candidates")
        if any_mode1:
            ref_out, ref_cand = ctx.match_ncc_full_dn(c.xyuvav, off, ocw, radius, 8, shift=sh, swap=swap)
            assert ctx.last_path() == path
            assert_bits_equal(ref_out, out, w + ": match_ncc_full_dn's record vs the class's own entry")
            assert_bits_equal(ref_cand, cand, w + ": match_ncc_full_dn's candidates vs the class's own entry")
            a_out, a_cand = ctx.match_ncc_full_any(c.xyuvav, off, ocw, radius, 8, shift=sh, swap=swap, mode=1)
            assert ctx.last_path() == "f32g_full"
            assert_bits_equal(a_out, ref_out, w + ": match_ncc_full_any(mode=1)'s record vs match_ncc_full_dn's")
            assert_bits_equal(a_cand, ref_cand, w + ": match_ncc_full_any(mode=1)'s candidates vs match_ncc_full_dn's")


@pytest.mark.parametrize("case", FULL_CASES, ids=case_id)
def test_exhaustive_search_at_the_top_of_the_class(api, case):
    kind, spread, ocw, null_frac, radius = case
    c, i0, i1 = class_pair(kind, spread, ocw, null_frac)
    any_mode1 = ocw == 40 and null_frac == 0.03 and spread == CLASSES[kind][1][0]        # one config per class
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        search_both_ways(api, ctx, kind, i0, i1, c, ocw, radius, case_id(case), any_mode1)


# ---- one null in an otherwise null-free pair ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocw", [30, 40])
def test_one_null_in_the_search_box_or_in_the_chip(api, ocw):
    """ocw 30 and 40 at R 15: search boxes of 91^2 and 111^2 pixels, both beyond one packed query.  tests/test_value_limits_cpu.py
    asserts that the null changes the oracle's record of exactly the points that see it."""
    c, i0, i1 = class_pair("u8", 1, ocw, 0.0)
    u, v = grid_uv(c.xyuvav)
    box_null = one_null(i1, int(u[6]) + ocw + 9, int(v[6]) - ocw - 6)             # in point 6's box, outside its chip-sized centre
    chip_null = one_null(i0, int(u[13]) + 3, int(v[13]) - 4)                      # in point 13's chip
    with api.Context(0) as ctx:
        for a, b, what in ((i0, box_null, "a null in the box"), (chip_null, i1, "a null in the chip"), (chip_null, box_null, "both")):
            ctx.set_images(a, b)
            search_both_ways(api, ctx, "u8", a, b, c, ocw, FULL_R, f"ocw {ocw}, {what}")


def test_one_null_in_a_dlc_window_on_either_side_of_8224_pixels(api, oracle):
    ocw = DLC_NULL_OCW
    c = base_pair(ocw, 0.0, DLC_NULL_SPEED, DLC_NULL_ANGLE)
    _, i0, i1 = class_pair("u8", 1, ocw, 0.0)
    H, W = i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    x, y, w, h = dlc_windows(c.xyuvav, c.offset, off, uv, ocw)
    px = w * h
    assert (px <= PACKED_QUERY_PIXELS).sum() >= 3 and (px > PACKED_QUERY_PIXELS).sum() >= 3
    u, v = grid_uv(c.xyuvav)
    modes = ("auto", "u8px", "u16")
    with api.Context(0) as ctx:
        for g in (int(np.flatnonzero(px <= PACKED_QUERY_PIXELS)[0]), int(np.flatnonzero(px > PACKED_QUERY_PIXELS)[0])):
            win_null = one_null(i1, int(u[g]) + int(c.offset[0]) + 4, int(v[g]) + int(c.offset[1]) - 5)
            chip_null = one_null(i0, int(u[g]) + 3, int(v[g]) - 4)
            for a, b, what in ((i0, win_null, "a null in the window"), (chip_null, i1, "a null in the chip")):
                ctx.set_images(a, b)
                dlc_both_ways(api, oracle, ctx, a, b, c, ocw, f"point {g} ({int(px[g])} window pixels), {what}", modes=modes)


@pytest.mark.parametrize("which", ["ocw40", "ocw30_diagonal"])
def test_null_free_windows_beyond_8224_pixels_are_classed_clean(which):
    """What a forgotten split costs inside the boxes the kernels ask for is a class, not a result: at the top of the 8-bit class one
    packed query over more than 8,224 pixels returns the null count plus a carry, so a null-free window reads as holding a null and its
    point leaves the clean list of the matrix-core step (the other forms return the same bytes, later).  u8_classify's own statistic
    (MIMC3_MX_STATS, read once per process: hence the child process) must call all 20 points of the null-free pair clean: windows of
    108 x 100 pixels at ocw 40; 90 x 90 and 92 x 92 at ocw 30 under the diagonal a-priori."""
    from u8_stats_common import stats_run
    ocw, grid = (40, "") if which == "ocw40" else (DLC_NULL_OCW, f", {DLC_NULL_SPEED}, {DLC_NULL_ANGLE}")
    body = (f"from value_limit_common import base_pair, class_pair; ocw = {ocw}; c = base_pair(ocw, 0.0{grid}); "
            f"i0, i1 = class_pair('u8', 1, ocw, 0.0)[1:]; xy, offset = c.xyuvav, c.offset; "
            f"off, uv = api.get_uv_pivot(xy, c.dt, c.mpp, ocw, *i0.shape)")
    c_clean, c_rest, c_nulls, c_wn, l_clean, l_rest, done, rest_after = stats_run(body)
    print(which, "classes clean", c_clean, "rest", c_rest, "nulls", c_nulls, "window-nulls", c_wn, "lists", l_clean, l_rest)
    assert (c_clean, c_rest, c_nulls, c_wn) == (20, 0, 0, 0) and (l_clean, l_rest) == (20, 0)


# ---- class edges ------------------------------------------------------------------------------------------------------------------------
EDGES = [("u8", 1, 256.0), ("12bit", 3, 4096.0), ("eighths", 3, 4096.0 / 8), ("20bit", 4095, float(2 ** 20))]


@pytest.mark.parametrize("ocw", [7, 40])
@pytest.mark.parametrize("kind,spread,above", EDGES, ids=[e[0] for e in EDGES])
def test_one_pixel_above_the_top_moves_the_pair_to_the_next_class(api, oracle, kind, spread, above, ocw):
    c, i0, i1 = class_pair(kind, spread, ocw, 0.03)
    u, v = grid_uv(c.xyuvav)
    raised = np.array(i1, np.float32)
    y, x = int(v[7]) - 1, int(u[7]) + 2                    # next to point 7: in its window, and in its chip when swapped
    assert raised[y, x] != 0 and above == CLASSES[kind][0] / CLASSES[kind][2] + 1 / CLASSES[kind][2]
    raised[y, x] = above
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        before = dlc_both_ways(api, oracle, ctx, i0, i1, c, ocw, f"{kind} ocw {ocw}, at the top", modes=("auto",))["auto"]
        ctx.set_images(i0, raised)
        after = dlc_both_ways(api, oracle, ctx, i0, raised, c, ocw, f"{kind} ocw {ocw}, one pixel above", modes=("auto", "general"))["auto"]
        print(f"{kind} ocw {ocw}: {before} -> {after}")
        assert (before, after) == {"u8": ("u8_mfma", "u8_offset"), "12bit": ("u8_offset", "f32_tiled"), "eighths": ("u16_scaled", "f32_tiled"),
                                   "20bit": ("f32_tiled", "f32_tiled")}[kind]
        shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
        if kind in ("12bit", "eighths"):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full_planes(c.xyuvav, c.offset, ocw, FULL_R, 8, shift=shift)
            assert e.value.code == -6
            search_both_ways(api, ctx, "16bit" if kind == "12bit" else "20bit_eighths", i0, raised, c, ocw, FULL_R, f"{kind} ocw {ocw}, one pixel above")
        elif kind == "20bit":
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full_dn(c.xyuvav, c.offset, ocw, FULL_R, 8, shift=shift)
            assert e.value.code == -6
            # the next class's entry still matches the pair: the float kernel against the float-pixel oracle (every f64 sum of this pair is
            # an integer below 2^53, exact in any order, so the comparison is on the bits here too)
            from full_any_common import full_any
            for swap in (False, True):
                sgn = -1 if swap else 1
                want_out, want = full_any(i0, raised, c.xyuvav, sgn * c.offset, ocw, FULL_R, 8, shift=sgn * shift, swap=swap)[:2]
                out, cand = ctx.match_ncc_full_any(c.xyuvav, sgn * c.offset, ocw, FULL_R, 8, shift=sgn * shift, swap=swap)
                assert ctx.last_path() == "f32g_full"
                assert_records_match(out, want_out, f"20bit ocw {ocw}, one pixel above, swap {swap}: match_ncc_full_any's record")
                assert_bits_equal(cand, want, f"20bit ocw {ocw}, one pixel above, swap {swap}: match_ncc_full_any's candidates")
        else:
            search_both_ways(api, ctx, "12bit", i0, raised, c, ocw, FULL_R, f"{kind} ocw {ocw}, one pixel above")
