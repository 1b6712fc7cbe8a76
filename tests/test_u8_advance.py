"""The advance list of the u8 matcher step on the GPU (u8_classify_kernel.hip, match_mx_kernel.hip, match_px_kernel.hip): window-null
points whose climb area (mx_climb_area, match_kernel.h) is null-free are tried by the matrix-core kernel's clean form before the
register-tiled launch, which skips those it finished.  Every result is path "auto" against the register-tiled kernel alone ("u8px")
and the CPU oracle, bit for bit, forward and swapped, through the device entry into a NaN-prefilled output; the list figures (length,
tried, finished) come from the kernels' diagnostics in a child process and are held against the numpy restatement of the rule
(tests/u8_advance_common.py).  Pairs of about (2 ocw + 230)^2 pixels, 30 to 80 points.

Not built, because it cannot exist: a point whose window is more than 80 % null with a null-free climb area.  The area holds the boxes
of every cell between pivot 0's and the last pivot's, which is never less than a third of the window
(test_area_is_never_a_fifth_of_the_window, no GPU needed), so the clean form's 0.8 rule cannot fire on an advance point; its branch
leaves the point to the register-tiled launch."""
import numpy as np
import pytest

import u8_advance_common as ac
from conftest import assert_bits_equal


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def run_dev(api, ctx, xy, offset, off, uv, ocw, swap):
    """one call of the device entry into an output prefilled with NaN"""
    from hipmem import DevArray
    d_xy, d_uv, d_off = DevArray(src=np.ascontiguousarray(xy, np.float64)), DevArray(src=np.ascontiguousarray(uv, np.int32)), DevArray(src=np.ascontiguousarray(off, np.int64))
    d_out = DevArray(src=np.full((len(xy), 3), np.nan, np.float32))
    ctx.matching_ncc_dlc_2_dev(d_xy.ptr, len(xy), offset, d_uv.ptr, d_off.ptr, api.pivot_extent(off, uv), ocw, d_out.ptr, swap=swap)
    out = d_out.numpy()
    for d in (d_xy, d_uv, d_off, d_out):
        d.free()
    return out


def check(api, ctx, oracle, case, what, with_oracle=True):
    """auto == u8px (== the oracle) in both directions; every point's status column was written"""
    i0, i1, xy, offset, off, uv, ocw = case
    offset = np.asarray(offset, np.int32)
    for swap in (False, True):
        o, p = (-offset, -uv) if swap else (offset, uv)
        ctx.set_path("auto")
        got = run_dev(api, ctx, xy, o, off, p, ocw, swap)
        assert ctx.last_path() == "u8_mfma", what
        ctx.set_path("u8px")
        assert_bits_equal(got, run_dev(api, ctx, xy, o, off, p, ocw, swap), f"{what} swap {swap}: auto vs u8px")
        if with_oracle:
            a, b = (i1, i0) if swap else (i0, i1)
            assert_bits_equal(got, oracle.match(a, b, xy, o, off, p, ocw), f"{what} swap {swap}: auto vs oracle")
    ctx.set_path("auto")


def n_advance(case):
    return int(ac.classify(*case)["advance"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", (7, 16, 40))
def test_borders_of_the_rule(api, oracle, ocw):
    """one planted null a pixel outside the area's rectangle (sides, corners): the point is on the list and finished; a pixel inside:
    it is not on the list.  ocw 40: the rectangle is beyond one packed table query"""
    spots = [(s, f) for f in (False, True) for s in ac.BORDER_SPOTS if ac.border_case(api, ocw, s, f)[1]]
    assert {s for s, _ in spots} == set(ac.BORDER_SPOTS)
    with api.Context(0) as ctx:
        for s, f in spots:
            case = ac.border_case(api, ocw, s, f)[0]
            ctx.set_images(case[0], case[1])
            check(api, ctx, oracle, case, f"{s} flip {f} ocw {ocw}", with_oracle=ocw != 40 or s in ("out_tl", "in_left"))
    stats = ac.advance_stats("cases = [ac.border_case(api, %d, s, f)[0] for s, f in %r]" % (ocw, spots))
    assert len(stats) == len(spots)
    for (s, f), st in zip(spots, stats):
        case, _, g = ac.border_case(api, ocw, s, f)
        k = ac.classify(*case)
        print(ocw, s, f, "numpy advance", int(k["advance"].sum()), "list, tried, finished", st[4:])
        assert st[4] == int(k["advance"].sum()) == st[5], (s, f, st)
        assert bool(k["advance"][g]) == s.startswith("out_")
        # a smooth null-free pair whose shift lies inside the corridor: every climb stays in its area
        assert st[6] == st[4], (s, f, st)
        assert st[1] == int((~k["clean"]).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", (7, 16))
def test_t4_areas_at_the_last_reachable_cells(api, oracle, ocw):
    case = ac.t4_case(api, ocw)
    with api.Context(0) as ctx:
        ctx.set_images(case[0], case[1])
        check(api, ctx, oracle, case, f"t4 ocw {ocw}")
    (st,) = ac.advance_stats("cases = [ac.t4_case(api, %d)]" % ocw)
    print("t4", ocw, st)
    assert st[4] == n_advance(case) == st[5] and 1 <= st[6] <= st[4]


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", (7, 16))
def test_climbs_that_leave_the_area(api, oracle, ocw):
    """a shift far off the corridor: advance points are tried and not finished; the rest list is as long as without them, and what the
    clean list hands on is what is classed kMxRest beyond it afterwards"""
    case = ac.off_corridor_case(api, ocw)
    assert n_advance(case) >= 4
    with api.Context(0) as ctx:
        ctx.set_images(case[0], case[1])
        check(api, ctx, oracle, case, f"off-corridor ocw {ocw}")
    (st,) = ac.advance_stats("cases = [ac.off_corridor_case(api, %d)]" % ocw)
    l_clean, l_rest, done, rest_after, n_adv, tried, fin = st
    k = ac.classify(*case)
    print("off-corridor", ocw, st)
    assert n_adv == int(k["advance"].sum()) == tried and tried > fin
    assert l_rest == int((~k["clean"]).sum()) and l_clean - done == rest_after - l_rest


def direct_case(api, ocw):
    """four far-apart points of a null-free pair with hand-made pivot lists, a null planted on each point's window pixel (0, 0) (never
    inside an area): two monotone lists, one that doubles back, and one (point 2) whose second pivot starts inside the window but outside
    the area -- its first scan is refused, so the point is never finished"""
    c = ac.small(ocw, 8900 + ocw, shift=(2, -1))
    xy = np.ascontiguousarray(c.xyuvav[[0, 5, 24, 29]])
    lists = [[(0, 0), (2, -1), (4, -2)], [(0, 0), (3, -2), (1, -1), (4, -3)], [(0, 0), (-4, 4), (6, -6)], [(k, -k // 2) for k in range(6)]]
    off = np.zeros(5, np.int64)
    off[1:] = np.cumsum([len(p) for p in lists])
    uv = np.ascontiguousarray(np.concatenate([np.array(p, np.int32) for p in lists]), np.int32)
    i1 = c.i1.copy()
    k = ac.classify(c.i0, i1, xy, c.offset, off, uv, ocw)
    for g in range(4):
        i1[k["wv"][g], k["wu"][g]] = 0.0
    return c.i0, i1, xy, c.offset, off, uv, ocw


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", (7, 16))
def test_pivot_lists_that_are_not_monotone(api, oracle, ocw):
    case = direct_case(api, ocw)
    k = ac.classify(*case)
    assert k["advance"].all()
    with api.Context(0) as ctx:
        ctx.set_images(case[0], case[1])
        check(api, ctx, oracle, case, f"direct pivots ocw {ocw}")
    (st,) = ac.advance_stats("import test_u8_advance as ta; cases = [ta.direct_case(api, %d)]" % ocw)
    print("direct pivots", ocw, st)
    assert st[4:6] == (4, 4) and 1 <= st[6] <= 3              # (point 2's pivot (-4, 4) starts outside its area: never finished)


def repeated_case(api, ocw, n):
    """n copies of one advance point (out_tl's target): a list of exactly n, and every rest point on it"""
    (i0, i1, xy, offset, off, uv, _), _, g = ac.border_case(api, ocw, "out_tl")
    p = uv[off[g]:off[g + 1]]
    off2 = np.arange(n + 1, dtype=np.int64) * len(p)
    return i0, i1, np.ascontiguousarray(np.repeat(xy[g:g + 1], n, axis=0)), offset, off2, np.ascontiguousarray(np.tile(p, (n, 1)), np.int32), ocw


@pytest.mark.gpu
def test_list_edges_and_switches(api, oracle, tmp_path):
    """list lengths 1, 63, 65 with every rest point on the list; an empty list while window-null points exist; either switch off:
    the same bytes and a length of 0"""
    with api.Context(0) as ctx:
        for n in (1, 63, 65):
            case = repeated_case(api, 16, n)
            assert n_advance(case) == n
            ctx.set_images(case[0], case[1])
            check(api, ctx, oracle, case, f"{n} copies", with_oracle=n == 1)
    body = ("import test_u8_advance as ta; cases = [ta.repeated_case(api, 16, n) for n in (1, 63, 65)] + "
            "[ac.border_case(api, 16, 'in_left')[0], ac.blobs_case(api, 16)]")
    on = ac.advance_stats(body, outdir=str(tmp_path / "on"))
    print("list edges", on)
    assert [(s[1], s[4], s[5], s[6]) for s in on[:3]] == [(n, n, n, n) for n in (1, 63, 65)]
    assert on[3][4] == 0 and on[3][1] > 0
    assert on[4][4] == n_advance(ac.blobs_case(api, 16)) > 0
    for name, env in (("advance_off", {"MIMC3_U8_ADVANCE": "0"}), ("records_off", {"MIMC3_U8_RECS": "0"})):
        off_ = ac.advance_stats(body, env=env, outdir=str(tmp_path / name))
        assert [s[4:] for s in off_] == [(0, 0, 0)] * 5, (name, off_)
        assert [s[1] for s in off_] == [s[1] for s in on]
        for i in range(5):
            assert_bits_equal(np.load(tmp_path / name / f"{i}.npy"), np.load(tmp_path / "on" / f"{i}.npy"), f"{name} call {i}")


@pytest.mark.gpu
def test_state_across_calls(api, oracle):
    """one context, pairs by turns whose rest positions are advance points in one and not in the other: a done bit left over from the
    call before would leave a NaN"""
    a, b, c = repeated_case(api, 16, 65), ac.border_case(api, 16, "in_left")[0], ac.blobs_case(api, 16)
    with api.Context(0) as ctx:
        for i, case in enumerate((a, b, c, a, c, b)):
            ctx.set_images(case[0], case[1])
            check(api, ctx, oracle, case, f"call {i}", with_oracle=False)


@pytest.mark.gpu
def test_two_matcher_lanes_back_to_back(api):
    """42,000 points through matching_ncc_dlc_cor (chunks on two streams and two matcher lanes: two advance lists), twice"""
    from mimc3_amd import synth
    ocw = 16
    c = synth.make_small(seed=8950, ocw=ocw, shift=(3, -2), angle_deg=25.0, speed=1500.0, h=1230, w=1280, dimx=210, dimy=200,
                         noise_dn=2, null_frac=0.02, margin=ocw + 40)
    off, uv = ac.pivots(api, c, ocw)
    assert n_advance((c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw)) > 1000
    cor = api.pivot_corridors(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        ctx.set_path("u8px")
        want = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, ocw)
        ctx.set_path("auto")
        for rep in range(2):
            assert_bits_equal(ctx.matching_ncc_dlc_cor(c.xyuvav, cor, c.offset, ocw), want, f"chunked call {rep}")
            assert ctx.last_path() == "u8_mfma"


def test_area_is_never_a_fifth_of_the_window():
    """no GPU: for every chip size and every last pivot whose set fits the tile, the area's pixel rectangle is more than 20 % of the
    window -- so no window can be more than 80 % null outside it, and the 0.8 rule cannot fire on an advance point"""
    for ocw in (7, 15, 16, 30, 32, 40):
        l = np.arange(-40, 41)
        fits, _, _, _, _, n = ac.axis_geometry(l, ocw)
        frac = n / (2.0 * (np.abs(l) + ocw + 2) + 1)
        f = frac[fits.astype(bool)]
        assert f.min() ** 2 > 0.2, (ocw, f.min())
