"""GPU: every matcher at every pixel phase of chip and window origin, and at fractional coordinates.

The fixtures of tests/phase_common.py (qualified on the CPU by tests/test_pixel_phases_cpu.py) hold all four chip phases in one launch
and are run at four control-point offsets, so every kernel form stages its chip and window rows at all 16 (chip phase, window phase)
pairs, with both row-end phases and with every null class -- and, in path mode auto, on the clean, advance and rest lists of the
matrix-core step.  Every comparison is on the bits (the records of the searches as tests/full_search_common.py compares them: the
SNR's f64 sum runs in another order on the device); last_path() is asserted in every case, so that no fallback stands in for the kernel
under test.

  * the DLC matcher (matching_ncc_dlc_2 against oracle.match) on 8-bit pairs in every path mode, on 9-bit, 12-bit, eighths and 16-bit
    pairs, forward and swapped; the many-pivot forms;
  * the exhaustive searches against each entry's oracle, with and without the a-priori shift, swapped once; boxes that end in the last
    rows and columns of the zero-bordered plane;
  * fractional coordinates (the reference truncates toward zero, MIMC_module.c:822-823): every entry returns the bytes it returns on
    the truncated grid, and the oracle's; the bounds at a fraction."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import full_any, tail_from_surface
from full_dn_common import full_dn
from full_multi_common import full_multi
from full_search_common import assert_records_match, full_search
from phase_common import BRIGHT_POINTS, OCWS, OFFSETS, SEARCH_R, fixture, fractional, many_pivot_fixture, plane_end_points, search_shifts, trunc
from value_limit_common import MODES, expected_path_at_limits, local_ranges

pytestmark = pytest.mark.gpu

U_OFFSETS = OFFSETS[:4]


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.fixture(autouse=True)
def records_as_shipped(monkeypatch):
    monkeypatch.delenv("MIMC3_U8_RECS", raising=False)


# ---- the DLC matcher -------------------------------------------------------------------------------------------------------------------
# pair -> (path modes, the kernel each must report)
DLC = {
    "u8": dict(zip(MODES, ("u8_mfma", "u8_exact", "u16_scaled", "f32_tiled", "general_f32"))),
    "9bit": {"auto": "u8_offset"},          # (the points whose chip or window holds the pixel of 500 come back through the u16 list)
    "12bit": {"auto": "u16_scaled"},
    "eighths": {"auto": "u16_scaled"},
    "16bit": {"auto": "f32_tiled", "general": "general_f32"},      # exact on integers: every f64 sum is an integer below 2^53
}


def dlc_at_every_offset(api, oracle, ctx, f, xy, modes, what, offsets=OFFSETS):
    off, uv = api.get_uv_pivot(xy, f.dt, f.mpp, f.ocw, *f.i0.shape)
    assert np.array_equal(off, f.off) and np.array_equal(uv, f.uv)
    for offset in offsets:
        offset = np.asarray(offset, np.int32)
        want = oracle.match(f.i0, f.i1, f.xy, offset, off, uv, f.ocw)
        want_sw = oracle.match(f.i1, f.i0, f.xy, -offset, off, -uv, f.ocw)
        for mode, path in modes.items():
            w = f"{what}, offset {offset.tolist()}, mode {mode}"
            ctx.set_path(mode)
            got = ctx.matching_ncc_dlc_2(xy, offset, off, uv, f.ocw)
            assert ctx.last_path() == path, w
            sw = ctx.matching_ncc_dlc_2(xy, -offset, off, -uv, f.ocw, swap=True)
            assert ctx.last_path() == path, w + ", swapped"
            assert_bits_equal(got, want, w)
            assert_bits_equal(sw, want_sw, w + ", swapped")
    ctx.set_path("auto")


@pytest.mark.parametrize("kind", list(DLC))
@pytest.mark.parametrize("ocw", OCWS)
def test_dlc_matcher_at_every_phase(api, oracle, ocw, kind):
    f = fixture(ocw, kind)
    for mode, path in DLC[kind].items():
        assert expected_path_at_limits(mode, f.i0, f.i1, ocw) == path, (mode, path)       # the fixture is of the class the table names
    if kind == "9bit":
        # the hand-over to the u16 list happens at every offset, in both directions: the chip or the window of every 16th point spans
        # more than a byte, and no other point's does (tests/test_pixel_phases_cpu.py asserts the same of the fixture)
        for offset in OFFSETS:
            for i0, i1, sgn in ((f.i0, f.i1, 1), (f.i1, f.i0, -1)):
                rc, rw = local_ranges(i0, i1, f.xy, sgn * np.asarray(offset), f.off, sgn * f.uv, ocw)
                wide = (rc > 254) | (rw > 254)
                assert np.array_equal(np.flatnonzero(wide), BRIGHT_POINTS), (offset, sgn)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        dlc_at_every_offset(api, oracle, ctx, f, f.xy, DLC[kind], f"ocw {ocw} {kind}")


@pytest.mark.parametrize("ocw,angle", [(15, 10.0), (30, 10.0)])
def test_many_pivot_forms_at_every_phase(api, oracle, ocw, angle):
    """more than 64 pivots per point: the forms of the register-tiled kernels that stage without tables"""
    f = many_pivot_fixture(ocw, angle)
    H, W = f.i0.shape
    off, uv = api.get_uv_pivot(f.xy, f.dt, f.mpp, ocw, H, W)
    assert np.diff(off).min() > 64 and len(set((trunc(f.xy)[0] & 3).tolist())) == 4
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for offset in U_OFFSETS:
            offset = np.asarray(offset, np.int32)
            want = oracle.match(f.i0, f.i1, f.xy, offset, off, uv, ocw)
            want_sw = oracle.match(f.i1, f.i0, f.xy, -offset, off, -uv, ocw)
            for mode, path in (("auto", "u8_exact"), ("u16", "u16_scaled")):
                ctx.set_path(mode)
                got = ctx.matching_ncc_dlc_2(f.xy, offset, off, uv, ocw)
                assert ctx.last_path() == path
                sw = ctx.matching_ncc_dlc_2(f.xy, -offset, off, -uv, ocw, swap=True)
                assert ctx.last_path() == path
                assert_bits_equal(got, want, f"ocw {ocw}, offset {offset.tolist()}, mode {mode}")
                assert_bits_equal(sw, want_sw, f"ocw {ocw}, offset {offset.tolist()}, mode {mode}, swapped")


# ---- the exhaustive searches --------------------------------------------------------------------------------------------------------------
NPEAKS = 4


def search_calls(f, offsets=OFFSETS):
    """(offset, shift, swap): every offset with the a-priori shift and without, and the first of each swapped"""
    prior, none = search_shifts(f)
    calls = [(np.asarray(o, np.int32), sh, False) for o in offsets for sh in (prior, none)]
    return calls + [(-np.asarray(offsets[1], np.int32), -prior, True), (-np.asarray(offsets[2], np.int32), none, True)]


def integer_images(f):
    """the pair as the integers the scaled-integer kernels keep (eighths: pixel * 8): what the integer oracles read"""
    s = np.float32(8) if f.kind == "eighths" else np.float32(1)
    return f.i0 * s, f.i1 * s


def check_integer_search(ctx, f, xy, radius, offset, shift, swap, what):
    """the entry of the pair's class against its oracle -> the results, for comparisons between calls"""
    ocw = f.ocw
    if f.kind == "u8":
        rec = ctx.match_ncc_full(xy, offset, ocw, radius, shift=shift, swap=swap)
        assert ctx.last_path() == "u8_mfma_full", what
        assert_records_match(rec, full_search(f.i0, f.i1, f.xy, offset, ocw, radius, shift=shift, swap=swap), what + ": match_ncc_full")
        out, cand = ctx.match_ncc_full_multi(xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap)
        assert ctx.last_path() == "u8_mfma_full", what
        assert_bits_equal(out, rec, what + ": match_ncc_full_multi's record vs match_ncc_full's")
        want_out, want = full_multi(f.i0, f.i1, f.xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap)
    elif f.kind in ("12bit", "eighths"):
        out, cand = ctx.match_ncc_full_planes(xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap)
        assert ctx.last_path() == "u16_full", what
        q0, q1 = integer_images(f)
        want_out, want = full_multi(q0, q1, f.xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap)
    else:
        out, cand = ctx.match_ncc_full_dn(xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap)
        assert ctx.last_path() == "f32i_full", what
        want_out, want = full_dn(f.i0, f.i1, f.xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap)
    assert_records_match(out, want_out, what + ": record")
    assert_bits_equal(cand, want, what + ": candidates")
    return out, cand


SEARCHES = [(ocw, SEARCH_R) for ocw in OCWS] + [(7, 15), (40, 15)]       # R 15 at ocw 40: the largest box, the split null count


@pytest.mark.parametrize("kind", ["u8", "12bit", "eighths", "16bit"])
@pytest.mark.parametrize("ocw,radius", SEARCHES, ids=[f"ocw{o}-R{r}" for o, r in SEARCHES])
def test_integer_searches_at_every_phase(api, ocw, radius, kind):
    """match_ncc_full and _full_multi on the matrix cores, _full_planes on the u16 planes (the clean kernel on the null-free points, the
    dirty one on the others), _full_dn on the f32 planes"""
    f = fixture(ocw, kind, plan="search")
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for offset, shift, swap in search_calls(f):
            check_integer_search(ctx, f, f.xy, radius, offset, shift, swap,
                                 f"ocw {ocw} {kind} R {radius}, offset {offset.tolist()}, shift {shift is not None}, swap {swap}")


def check_float_search(ctx, f, xy, radius, offset, shift, swap, what, wide=False):
    """match_ncc_full_any(mode=1) or match_ncc_wide on an integer pair: the surface is the oracle's bit for bit, record and candidates
    the oracle's tail of it"""
    ocw = f.ocw
    want_rec, _, want_surf, _ = full_any(f.i0, f.i1, f.xy, offset, ocw, radius, 0, shift=shift, swap=swap)
    if wide:
        rec, cand, surf = ctx.match_ncc_wide(xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap, surface=True)
        assert ctx.last_path() == ("f32g_wide" if radius >= 16 else "f32g_full"), what
    else:
        rec, cand, surf = ctx.match_ncc_full_any(xy, offset, ocw, radius, NPEAKS, shift=shift, swap=swap, mode=1, surface=True)
        assert ctx.last_path() == "f32g_full", what
    st3 = want_rec[:, 2] == -3
    assert np.array_equal(rec[:, 2] == -3, st3), what + ": status -3 points"
    assert_bits_equal(surf, want_surf, what + ": surface vs the oracle")
    t_rec, t_cand = tail_from_surface(surf, shift, radius, NPEAKS, refused=st3, device_snr_order=True)
    assert_bits_equal(rec, t_rec, what + ": record vs the tail of the surface")
    assert_bits_equal(cand, t_cand, what + ": candidates vs the tail of the surface")
    return rec, cand, surf


def float_calls(f):
    """the four offsets with the a-priori shift, once without, once swapped (the oracle of the float searches is the slow one)"""
    prior, none = search_shifts(f)
    return [(np.asarray(o, np.int32), prior, False) for o in U_OFFSETS] + [(np.asarray(OFFSETS[4], np.int32), none, False),
                                                                            (-np.asarray(OFFSETS[1], np.int32), -prior, True)]


@pytest.mark.parametrize("kind", ["u8", "12bit", "16bit"])
@pytest.mark.parametrize("ocw,radius", SEARCHES, ids=[f"ocw{o}-R{r}" for o, r in SEARCHES])
def test_float_search_at_every_phase(api, ocw, radius, kind):
    f = fixture(ocw, kind, plan="search")
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for offset, shift, swap in float_calls(f):
            check_float_search(ctx, f, f.xy, radius, offset, shift, swap,
                               f"ocw {ocw} {kind} R {radius}, offset {offset.tolist()}, shift {shift is not None}, swap {swap}")


WIDE = [(ocw, 16) for ocw in OCWS] + [(7, 31)]


@pytest.mark.parametrize("kind", ["u8", "12bit", "16bit"])
@pytest.mark.parametrize("ocw,radius", WIDE, ids=[f"ocw{o}-R{r}" for o, r in WIDE])
def test_wide_search_at_every_phase(api, ocw, radius, kind):
    f = fixture(ocw, kind, plan="search")
    assert radius <= api.wide_max_radius(ocw)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for offset, shift, swap in float_calls(f):
            check_float_search(ctx, f, f.xy, radius, offset, shift, swap,
                               f"wide ocw {ocw} {kind} R {radius}, offset {offset.tolist()}, shift {shift is not None}, swap {swap}", wide=True)


@pytest.mark.parametrize("ocw,radius", [(7, SEARCH_R), (16, SEARCH_R), (40, 15)])
def test_search_boxes_that_end_in_the_last_rows_and_columns_of_the_plane(api, ocw, radius):
    """A check that nothing faults and nothing is disturbed, not a check of values.  The matrix-core kernel's tile reaches past the search
    box, and its loads are clamped to the plane (tlim, issued before any refusal): two points whose box ends in the plane's last row, or
    in its last column at the last of the four offsets, among the fixture's points.  A box that reaches the end of the plane lies wholly
    in the zero border (the border is 256 pixels, the largest box 111), so these two points are refused with -3 whatever the clamped
    loads bring; no accepted point can reach tlim.  What is compared is every other point's record, which must be what it is without
    them."""
    f = fixture(ocw, "u8", plan="search")
    exy, eshift = plane_end_points(f, radius)
    prior = search_shifts(f)[0]
    xy, shift = np.ascontiguousarray(np.concatenate([f.xy, exy])), np.ascontiguousarray(np.concatenate([prior, eshift]), np.int32)
    H, W = f.i0.shape
    u0, v0 = trunc(exy)
    assert int(v0[0] + eshift[0, 1]) + radius + ocw == H + 255 and int(u0[1] + eshift[1, 0]) + 3 + radius + ocw == W + 255      # the last row, the last column
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for offset in U_OFFSETS:
            offset = np.asarray(offset, np.int32)
            rec = ctx.match_ncc_full(xy, offset, ocw, radius, shift=shift)
            assert ctx.last_path() == "u8_mfma_full"
            assert_records_match(rec, full_search(f.i0, f.i1, xy, offset, ocw, radius, shift=shift), f"ocw {ocw} R {radius}, offset {offset.tolist()}")
            assert (rec[-2:, 2] == -3).all()


# ---- fractional coordinates --------------------------------------------------------------------------------------------------------------
FR_OCW = 16
FR_OFFSET = np.array([1, -1], np.int32)


@pytest.mark.parametrize("kind", list(DLC))
def test_dlc_matcher_truncates(api, oracle, kind):
    f = fixture(FR_OCW, kind)
    fr = fractional(f.xy, 1)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        dlc_at_every_offset(api, oracle, ctx, f, fr, DLC[kind], f"{kind}, fractional grid", offsets=(OFFSETS[1], OFFSETS[4]))
        want = oracle.match(f.i0, f.i1, f.xy, FR_OFFSET, f.off, f.uv, FR_OCW)
        want_sw = oracle.match(f.i1, f.i0, f.xy, -FR_OFFSET, f.off, -f.uv, FR_OCW)
        cor = api.pivot_corridors(fr, f.dt, f.mpp)
        assert cor.tobytes() == api.pivot_corridors(f.xy, f.dt, f.mpp).tobytes()
        for mode, path in DLC[kind].items():
            ctx.set_path(mode)
            for xy, what in ((fr, "fractional"), (f.xy, "truncated")):
                assert_bits_equal(ctx.matching_ncc_dlc_geo(xy, FR_OFFSET, f.dt, f.mpp, FR_OCW), want, f"{kind} {mode}: dlc_geo, {what}")
                assert ctx.last_path() == path
                assert_bits_equal(ctx.matching_ncc_dlc_geo(xy, -FR_OFFSET, f.dt, f.mpp, FR_OCW, swap=True), want_sw, f"{kind} {mode}: dlc_geo swapped, {what}")
                assert_bits_equal(ctx.matching_ncc_dlc_cor(xy, cor, FR_OFFSET, FR_OCW), want, f"{kind} {mode}: dlc_cor, {what}")
                assert ctx.last_path() == path


@pytest.mark.parametrize("kind", ["u8", "12bit", "eighths", "16bit"])
def test_searches_truncate(api, kind):
    f = fixture(FR_OCW, kind, plan="search")
    fr = fractional(f.xy, 2)
    prior = search_shifts(f)[0]
    assert np.array_equal(api.prior_shift(fr, f.dt, f.mpp), prior)
    what = f"{kind}, fractional grid"
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            a = check_integer_search(ctx, f, fr, SEARCH_R, sgn * FR_OFFSET, sgn * prior, swap, what)
            b = check_integer_search(ctx, f, f.xy, SEARCH_R, sgn * FR_OFFSET, sgn * prior, swap, what + " (truncated)")
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), what + ": bytes of the call on the truncated grid"
            if kind != "eighths":
                for wide, radius in ((False, SEARCH_R), (True, 16)):
                    a = check_float_search(ctx, f, fr, radius, sgn * FR_OFFSET, sgn * prior, swap, what, wide=wide)
                    b = check_float_search(ctx, f, f.xy, radius, sgn * FR_OFFSET, sgn * prior, swap, what + " (truncated)", wide=wide)
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), what + ": bytes of the call on the truncated grid"


@pytest.mark.parametrize("kind,mode,path", [("u8", 0, "u8_mfma_full"), ("12bit", 0, "u16_full"), ("16bit", 0, "f32i_full"), ("u8", 1, "f32g_full")])
def test_forward_backward_truncates(api, kind, mode, path):
    """the rows of the backward search are built on the device from (int) u, (int) v (fb_kernel.hip)"""
    from full_fb_common import fb_chain, oracle_search
    f = fixture(FR_OCW, kind, plan="search")
    fr = fractional(f.xy, 3)
    H, W = f.i0.shape
    prior = search_shifts(f)[0]
    q0, q1 = integer_images(f)
    _, w_cand, w_fb, _ = fb_chain(oracle_search(q0, q1), f.xy, FR_OFFSET, FR_OCW, SEARCH_R, H, W, npeaks=3, shift=prior)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        out, cand, fb = ctx.match_ncc_full_fb(fr, FR_OFFSET, FR_OCW, SEARCH_R, 3, shift=prior, mode=mode)
        assert ctx.last_path() == path
        out_t, cand_t, fb_t = ctx.match_ncc_full_fb(f.xy, FR_OFFSET, FR_OCW, SEARCH_R, 3, shift=prior, mode=mode)
    assert out.tobytes() == out_t.tobytes() and cand.tobytes() == cand_t.tobytes() and fb.tobytes() == fb_t.tobytes()
    assert_bits_equal(cand, w_cand, f"{kind} mode {mode}: candidates vs the oracle")
    assert_bits_equal(fb, w_fb, f"{kind} mode {mode}: fb vs the oracle chain")


@pytest.mark.parametrize("kind", ["u8", "12bit", "16bit"])
def test_pyramids_truncate(api, kind):
    """the coarser levels take (int) u >> level (pyramid_kernel.hip)"""
    from pyramid_any_oracle import pyramid_search_any
    from pyramid_dn_oracle import pyramid_search_dn
    from pyramid_oracle import pyramid_search
    f = fixture(FR_OCW, kind, plan="search")
    fr = fractional(f.xy, 4)
    prior = search_shifts(f)[0]
    L = 2
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        if kind == "u8":
            rec, sh = ctx.match_ncc_pyramid(fr, FR_OFFSET, FR_OCW, SEARCH_R, L, shift=prior)
            assert ctx.last_path() == "u8_mfma_full"
            rec_t, sh_t = ctx.match_ncc_pyramid(f.xy, FR_OFFSET, FR_OCW, SEARCH_R, L, shift=prior)
            assert rec.tobytes() == rec_t.tobytes() and np.array_equal(sh, sh_t)
            w_rec, w_sh = pyramid_search(f.i0, f.i1, f.xy, FR_OFFSET, FR_OCW, SEARCH_R, L, shift=prior)
            assert np.array_equal(sh, w_sh)
            assert_records_match(rec, w_rec, "match_ncc_pyramid, fractional grid")
        got = ctx.match_ncc_pyramid_dn(fr, FR_OFFSET, FR_OCW, SEARCH_R, L, NPEAKS, shift=prior)
        assert ctx.last_path() == {"u8": "u8_mfma_full", "12bit": "u16_full", "16bit": "f32i_full"}[kind]
        got_t = ctx.match_ncc_pyramid_dn(f.xy, FR_OFFSET, FR_OCW, SEARCH_R, L, NPEAKS, shift=prior)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, got_t))
        want = pyramid_search_dn(f.i0, f.i1, f.xy, FR_OFFSET, FR_OCW, SEARCH_R, L, NPEAKS, shift=prior)
        assert np.array_equal(got[2], want[2])
        assert_records_match(got[0], want[0], f"match_ncc_pyramid_dn {kind}, fractional grid")
        assert_bits_equal(got[1], want[1], f"match_ncc_pyramid_dn {kind}, fractional grid: candidates")
        anyg = ctx.match_ncc_pyramid_any(fr, FR_OFFSET, FR_OCW, SEARCH_R, L, NPEAKS, shift=prior, mode=1)
        assert ctx.last_path() == "f32g_full"
        anyt = ctx.match_ncc_pyramid_any(f.xy, FR_OFFSET, FR_OCW, SEARCH_R, L, NPEAKS, shift=prior, mode=1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(anyg, anyt))
        wany = pyramid_search_any(f.i0, f.i1, f.xy, FR_OFFSET, FR_OCW, SEARCH_R, L, NPEAKS, shift=prior)
        und = wany[3]                                           # (points whose coarse peak the float levels' rounding may move)
        assert np.array_equal(anyg[2][~und], wany[2][~und]), "match_ncc_pyramid_any: shift_out vs the oracle"


def test_stack_truncates(api):
    f = fixture(FR_OCW, "u8", plan="search")
    fr = fractional(f.xy, 0)
    prior = search_shifts(f)[0]
    n = f.xy.shape[0]
    want_surf = full_any(f.i0, f.i1, f.xy, FR_OFFSET, FR_OCW, SEARCH_R, 0, shift=prior)[2]
    res = []
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for xy in (fr, f.xy):
            ctx.stack_begin(n, SEARCH_R, shift=prior)
            ctx.stack_add(xy, FR_OFFSET, FR_OCW)
            res.append(ctx.stack_finish(NPEAKS, surface=True))
        ctx.stack_begin(0, SEARCH_R)
    (out, cand, count, surf), (out_t, cand_t, count_t, surf_t) = res
    assert out.tobytes() == out_t.tobytes() and cand.tobytes() == cand_t.tobytes() and surf.tobytes() == surf_t.tobytes()
    assert np.array_equal(count, count_t) and (count == 1).all()
    assert_bits_equal(surf, want_surf, "one layer's mean surface vs the oracle's surface")


def test_control_point_offset_on_a_fractional_grid(api, oracle):
    """get_offset_image's candidates are xyuvav rows: status, offset, flags, counts and the f32 vote sums of the oracle on the same
    fractional grid"""
    from test_cp_offset_parity import CASES, K, cp_case
    i0, i1, xy = cp_case(**CASES["clean"])
    fr = fractional(xy, 1)
    rc, off, flag, info, sduv = oracle.get_offset_image(i0, i1, fr, K, 3, num_cp_min=20)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        st, o2, f2, info2, sduv2 = ctx.get_offset_image(fr, K, seed=3, num_cp_min=20)
    assert st == rc and np.array_equal(info2, info) and np.array_equal(f2, flag) and np.array_equal(o2, off)
    assert np.array_equal(sduv2.view(np.uint32), sduv.view(np.uint32)), (sduv2, sduv)


# ---- bounds at a fraction -------------------------------------------------------------------------------------------------------------------
DIMX_ROW = 8 * 3          # a point of the fixture's fourth row: its v is far from the image's top and bottom


def bound_points(f, us, v=None):
    """the fixture's first row of values with u replaced: points at the image's left and right bounds"""
    xy = np.array(f.xy[:len(us)], np.float64)
    xy[:, 2] = us
    if v is not None:
        xy[:, 3] = v
    xy[:, 0], xy[:, 1] = xy[:, 2] * f.mpp, -xy[:, 3] * f.mpp
    return np.ascontiguousarray(xy)


@pytest.mark.parametrize("ocw", [7, 16, 40])
def test_bounds_at_a_fraction(api, oracle, ocw):
    """u = ocw + 0.9 and u = W - 1 - ocw + 0.9 truncate to the first and the last chip that fits: accepted, and the oracle's result.
    u = ocw - 0.1 truncates to ocw - 1: the host entries refuse it with code -2.  (All of these stay inside every buffer: the planes
    carry a zero border of 256 pixels.)"""
    f = fixture(ocw, "u8", plan="search")
    H, W = f.i0.shape
    v = float(trunc(f.xy)[1][DIMX_ROW]) + 0.5
    ok = bound_points(f, [ocw + 0.9, W - 1 - ocw + 0.9], v)
    bad = bound_points(f, [ocw - 0.1, ocw + 0.9], v)
    okt = ok.copy(); okt[:, 2:4] = np.trunc(ok[:, 2:4])
    zero = np.zeros(2, np.int32)
    piv_off, piv_uv = np.array([0, 1, 2], np.int64), np.zeros((2, 2), np.int32)       # one pivot each: the corridor ends at the edge
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for mode in MODES:
            ctx.set_path(mode)
            assert_bits_equal(ctx.matching_ncc_dlc_2(ok, zero, piv_off, piv_uv, ocw), oracle.match(f.i0, f.i1, okt, zero, piv_off, piv_uv, ocw), f"dlc, {mode}")
            assert ctx.last_path() == DLC["u8"][mode]
            with pytest.raises(api.Mimc3Error) as e:
                ctx.matching_ncc_dlc_2(bad, zero, piv_off, piv_uv, ocw)
            assert e.value.code == -2
        ctx.set_path("auto")
        rec = ctx.match_ncc_full(ok, zero, ocw, SEARCH_R)
        assert ctx.last_path() == "u8_mfma_full"
        assert_records_match(rec, full_search(f.i0, f.i1, okt, zero, ocw, SEARCH_R), "match_ncc_full at the bounds")
        out, cand, surf = ctx.match_ncc_full_any(ok, zero, ocw, SEARCH_R, NPEAKS, mode=1, surface=True)
        assert_bits_equal(surf, full_any(f.i0, f.i1, okt, zero, ocw, SEARCH_R, 0)[2], "match_ncc_full_any at the bounds")
        for call in (lambda: ctx.match_ncc_full(bad, zero, ocw, SEARCH_R), lambda: ctx.match_ncc_full_multi(bad, zero, ocw, SEARCH_R, NPEAKS),
                     lambda: ctx.match_ncc_full_planes(bad, zero, ocw, SEARCH_R, NPEAKS), lambda: ctx.match_ncc_full_dn(bad, zero, ocw, SEARCH_R, NPEAKS),
                     lambda: ctx.match_ncc_full_any(bad, zero, ocw, SEARCH_R, NPEAKS, mode=1), lambda: ctx.match_ncc_wide(bad, zero, ocw, 16, NPEAKS),
                     lambda: ctx.match_ncc_full_fb(bad, zero, ocw, SEARCH_R, NPEAKS)):
            with pytest.raises(api.Mimc3Error) as e:
                call()
            assert e.value.code == -2



@pytest.mark.parametrize("kind", ["u8", "12bit", "16bit"])
def test_dev_entries_answer_a_chip_outside_the_image_with_nan(api, kind):
    """u = ocw - 0.1 through the _dev entries, which make no host check: the all-NaN record, the same on every kernel, and the
    neighbouring point's record untouched by it"""
    from hipmem import DevArray
    ocw = FR_OCW
    f = fixture(ocw, kind, plan="search")
    v = float(trunc(f.xy)[1][DIMX_ROW]) + 0.5
    xy = bound_points(f, [ocw - 0.1, ocw + 0.9], v)
    n = 2
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        d_xy = DevArray(src=xy)
        entries = {"u8": [("match_ncc_full", "u8_mfma_full", False), ("match_ncc_full_multi", "u8_mfma_full", True)],
                   "12bit": [("match_ncc_full_planes", "u16_full", True)], "16bit": [("match_ncc_full_dn", "f32i_full", True)]}[kind]
        entries += [("match_ncc_full_any", "f32g_full", True), ("match_ncc_wide", "f32g_wide", True)]
        for name, path, has_cand in entries:
            radius = 16 if name == "match_ncc_wide" else SEARCH_R
            d_out, d_cand = DevArray((n, 8), np.float32), DevArray((NPEAKS, n, 3), np.float32)
            dev = getattr(ctx, name + "_dev")
            if not has_cand:
                dev(d_xy.ptr, n, (0, 0), ocw, radius, d_out.ptr)
            elif name == "match_ncc_full_any":
                dev(d_xy.ptr, n, (0, 0), ocw, radius, NPEAKS, d_out.ptr, d_cand.ptr, mode=1)
            else:
                dev(d_xy.ptr, n, (0, 0), ocw, radius, NPEAKS, d_out.ptr, d_cand.ptr)
            out = d_out.numpy()
            assert ctx.last_path() == path, name
            assert np.isnan(out[0]).all(), f"{name}: the record of a chip outside the image"
            if has_cand:
                assert np.isnan(d_cand.numpy()[:, 0]).all(), f"{name}: its candidates"
            host = getattr(ctx, name)
            args = (xy[1:], (0, 0), ocw, radius) + ((NPEAKS,) if has_cand else ())
            want = host(*args, mode=1) if name == "match_ncc_full_any" else host(*args)
            assert_bits_equal(out[1:], want if not has_cand else want[0], f"{name}: the next point's record")
