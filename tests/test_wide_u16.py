"""GPU: the exhaustive search beyond +-15 px on scaled-integer pairs (12-bit DN, filtered 8-bit pairs) at any chip half-width 1..80 on
the matrix cores (mimc3_match_ncc_wide_planes, match_wide_u16_kernel.hip).

At the six built chip sizes mode 1 is compared byte for byte with match_ncc_wide on the same 12-bit pair (the float wide kernel: both hold
exact integer sums and use the same finish); everywhere with the oracle of tests/full_any_common.py: the surface bit for bit (a
non-finite cell of the same kind), record and candidates against the oracle's tail of the device surface AND of the oracle surface.  The
fixtures are those of tests/wide_u16_common.py (tests/test_wide_u16_cpu.py counts them): 12 points whose boxes do not overlap -- nulls in
the box only (its last row, its last column, inside one tile's window alone), in the chip only, on both sides, one column outside the
box, a status -4 in the last partial tile, a status -3 by the chip rule and one by the box rule, clean points.  No comparison here has a
tolerance: every one is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import full_chip_u8_common as fu
import wide_u16_common as wp
from conftest import assert_bits_equal
from full_any_common import full_any, tail_from_surface, to_float
from full_chip_u16_common import filtered_pair, spread12
from full_dn_common import to_dn16
from wide_common import FAR_R, FAR_TRUE, far_case

pytestmark = pytest.mark.gpu
PEAKS = (0, 1, 4, 8)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def same_surface(got, want, what):
    """finite cells bit for bit, a non-finite cell of the same kind"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what + ": finite cells differ"
    assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]), what + ": finite cells are not bit-equal"
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(got)], want[~fin & ~np.isnan(want)]), what + ": kinds"


def vs_oracle(got, pts, o_rec, o_surf, shift, radius, npeaks, what):
    """record, candidates and surface of the points `pts` against the oracle's record and surfaces"""
    rec, cand, surf = got[0][pts], None if got[1] is None else got[1][:, pts], got[2][pts]
    sh = None if shift is None else shift[pts]
    st3 = o_rec[:, 2] == -3
    same_surface(surf, o_surf, what + ": surface vs the oracle")
    assert np.isnan(surf[st3]).all() and np.array_equal(rec[:, 2] == -3, st3)
    for name, s in (("device", surf), ("oracle", o_surf)):
        t_rec, t_cand = tail_from_surface(s, sh, radius, npeaks, refused=st3, device_snr_order=True)
        assert_bits_equal(rec, t_rec, f"{what}: record vs the tail of the {name} surface")
        if npeaks:
            assert_bits_equal(cand, t_cand, f"{what}: candidates vs the tail of the {name} surface")
    for k in (-2, -3, -4):
        assert np.array_equal(rec[:, 2] == k, o_rec[:, 2] == k), f"{what}: status {k}"


def run(ctx, f, npeaks, mode=1, surface=True, path=wp.PATH):
    got = ctx.match_ncc_wide_planes(f["xy"], f["off"], f["ocw"], f["R"], npeaks, shift=f["shift"], swap=f["swap"], mode=mode, surface=surface)
    assert ctx.last_path() == path
    return got


def vs_wide(ctx, f, got, npeaks, what):
    ref = ctx.match_ncc_wide(f["xy"], f["off"], f["ocw"], f["R"], npeaks, shift=f["shift"], swap=f["swap"], surface=True)
    assert ctx.last_path() == wp.FLOAT_PATH
    same_surface(got[2], ref[2], what + ": surface vs match_ncc_wide")
    assert_bits_equal(got[0], ref[0], what + ": record vs match_ncc_wide")
    if npeaks:
        assert_bits_equal(got[1], ref[1], what + ": candidates vs match_ncc_wide")


def check_fixture(api, fx, six, peaks=PEAKS):
    f = wp.fixture(*fx)
    pts, o_rec, o_surf = wp.oracle(*fx)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in peaks:
            got = run(ctx, f, npeaks)
            what = f"{f['what']}, npeaks {npeaks}"
            assert (got[1] is None) == (npeaks == 0)
            vs_oracle(got, pts, o_rec, o_surf, f["shift"], f["R"], npeaks, what)
            if six:
                vs_wide(ctx, f, got, npeaks, what)
            bare = run(ctx, f, npeaks, surface=False)
            assert_bits_equal(bare[0], got[0], what + ": record without surfaces")
            if npeaks:
                assert_bits_equal(bare[1], got[1], what + ": candidates without surfaces")
    rec, surf = got[0], got[2]
    assert rec[wp.G4, 2] == -4 and rec[wp.G3CHIP, 2] == -3 and rec[wp.G3BOX, 2] == -3
    ok = np.setdiff1d(np.arange(rec.shape[0]), [wp.G3CHIP, wp.G3BOX])
    assert np.isfinite(surf[ok]).all() and (rec[ok, 2] >= -1).sum() >= 8
    return rec, surf


# ---- 1. mode 1 at the six: the bytes of match_ncc_wide on the same 12-bit pair (and of the oracle) ----
@pytest.mark.parametrize("ocw,radius", wp.SIX_CASES)
def test_mode1_at_the_six_is_match_ncc_wide(api, ocw, radius):
    check_fixture(api, (ocw, radius, "dn12", False, True), six=True)


@pytest.mark.parametrize("swap,with_shift", [(True, True), (False, False)])
def test_direction_and_shift_at_16(api, swap, with_shift):
    check_fixture(api, (16, 23, "dn12", swap, with_shift), six=True, peaks=(0, 8))


# ---- 2. mode 1 outside the six: the oracle ----
@pytest.mark.parametrize("ocw,radius", wp.OUTSIDE_CASES)
def test_mode1_outside_the_six_is_the_oracle(api, ocw, radius):
    check_fixture(api, (ocw, radius, "dn12", False, True), six=False, peaks=PEAKS if ocw < 45 else (0, 8))


@pytest.mark.parametrize("ocw,radius", [(10, 24), (57, 16)])
def test_swapped_outside_the_six(api, ocw, radius):
    check_fixture(api, (ocw, radius, "dn12", True, True), six=False, peaks=(0, 4))


# ---- 3. the placed nulls are finished points with the oracle's bytes (checked above); here: what each one is ----
def test_placed_nulls(api):
    rec, surf = check_fixture(api, (24, 47, "dn12", False, True), six=False, peaks=(0,))
    for g in fu.BOX_ONLY + fu.CHIP_ONLY + fu.BOTH + (wp.OUTSIDE, wp.ONE_TILE):
        assert np.isfinite(surf[g]).all() and rec[g, 2] >= -1


# ---- 4. saturated 12-bit pairs: the integer bounds, the sub-box table sums (44 | 45), the finish's rounding products (80) ----
@pytest.mark.parametrize("ocw,radius", wp.SATURATED)
@pytest.mark.parametrize("kind", ["sat3", "sat63"])
def test_saturated(api, ocw, radius, kind):
    check_fixture(api, (ocw, radius, kind, False, True), six=False, peaks=(0, 4))


# ---- 5. scale 8 on both images and on one; an 8-bit pair on its u16 planes ----
@pytest.mark.parametrize("kind", ["eighths", "mixed"])
def test_eighths_and_the_mixed_scale(api, kind):
    check_fixture(api, (10, 24, kind, False, True), six=False, peaks=(0, 4))


@pytest.mark.parametrize("ocw,radius", [(16, 24), (10, 24), (57, 16)])
def test_mode1_on_an_8bit_pair_is_the_u8_kernels_bytes(api, ocw, radius):
    import wide_u8_common as wu
    f = wu.fixture(ocw, radius, False, True, 0)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in (0, 4):
            want = ctx.match_ncc_wide_class(f["xy"], f["off"], ocw, radius, npeaks, shift=f["shift"], mode=1, surface=True)
            assert ctx.last_path() == wp.U8_PATH
            got = run(ctx, f, npeaks)
            assert same_bytes(got, want), f"ocw {ocw} R {radius} npeaks {npeaks}"


# ---- 6. the filtered forms of an 8-bit pair ----
@pytest.mark.parametrize("ocw", [16, 10])
@pytest.mark.parametrize("which", [0, 2], ids=["ddx", "laplacian"])
def test_filtered_pairs(api, ocw, which):
    import wide_u8_common as wu
    radius = 24
    f = wu.fixture(ocw, radius, False, True, 0)
    pts = np.arange(f["xy"].shape[0])
    with api.Context(0) as ctx:
        f0, f1 = filtered_pair(ctx, api, which, f["i0"], f["i1"])
        o_rec, _, o_surf, _ = full_any(f0, f1, f["xy"], f["off"], ocw, radius, 0, shift=f["shift"])
        for npeaks in (0, 4):
            got = run(ctx, f, npeaks)
            what = f"filter {which} ocw {ocw} npeaks {npeaks}"
            vs_oracle(got, pts, o_rec, o_surf, f["shift"], radius, npeaks, what)
            assert same_bytes(run(ctx, f, npeaks, mode=0), got), what + ": mode 0"
            if ocw == 16:
                vs_wide(ctx, f, got, npeaks, what)


# ---- 7. seams ----
def seam_check(api, p0, p1, xy, radius, what):
    o_rec, _, o_surf, _ = full_any(p0, p1, xy, (0, 0), wp.SEAM_OCW, radius, 0)
    pts = np.arange(xy.shape[0])
    with api.Context(0) as ctx:
        ctx.set_images(p0, p1)
        for npeaks in (0, 8):
            got = ctx.match_ncc_wide_planes(xy, (0, 0), wp.SEAM_OCW, radius, npeaks, mode=1, surface=True)
            assert ctx.last_path() == wp.PATH
            vs_oracle(got, pts, o_rec, o_surf, None, radius, npeaks, f"{what}, npeaks {npeaks}")
            ref = ctx.match_ncc_wide(xy, (0, 0), wp.SEAM_OCW, radius, npeaks, surface=True)
            assert same_bytes(got, ref), what + ": vs match_ncc_wide"
    return got


@pytest.mark.parametrize("period", wp.SEAM_PERIODS)
def test_tied_maxima_across_tiles(api, period):
    """exactly tied maxima in every cell tile, at the cells 31 and 63 / 32 and 64: first-wins in k, and the local-maximum rule reads
    neighbours across the seams"""
    p0, p1, xy = wp.seam_pair(*period, plateau=False)
    rec, cand, surf = seam_check(api, p0, p1, xy, wp.SEAM_R, f"periodic {period}")
    S = 2 * wp.SEAM_R + 1
    xs, ys = wp.maxima_cells(period[0]), wp.maxima_cells(period[1])
    want = sorted(x * S + y for x in xs for y in ys)[:8]
    for g in range(xy.shape[0]):
        assert (cand[:, g, 2] == cand[0, g, 2]).all() and rec[g, 2] == cand[0, g, 2]
        k = [int(round(cand[j, g, 0] + wp.SEAM_R)) * S + int(round(cand[j, g, 1] + wp.SEAM_R)) for j in range(8)]
        assert k == want, (g, k, want)


@pytest.mark.parametrize("radius,y", wp.SEAM_PLATEAUS)
def test_plateau_across_a_seam(api, radius, y):
    p0, p1, xy = wp.seam_pair(*wp.PLATEAU_PERIOD, plateau=True)
    rec, cand, surf = seam_check(api, p0, p1, xy[:3], radius, f"plateau R {radius}")
    S = 2 * radius + 1
    v = surf[0].reshape(S, S)
    assert v[radius, y] == v[radius, y + 1] == v.max()


# ---- 8. what it is for: the displaced pair as 12-bit DN, at a built chip size and at one that is not ----
@pytest.mark.parametrize("ocw", [16, 10])
def test_displacement_beyond_15_px(api, ocw):
    c = far_case()
    with api.Context(0) as ctx:
        ctx.set_images(spread12(c.i0), spread12(c.i1))
        for mode in (0, 1):
            far, _ = ctx.match_ncc_wide_planes(c.xyuvav, (0, 0), ocw, FAR_R, 0, mode=mode)
            assert ctx.last_path() == wp.PATH
            assert np.isfinite(far[:, 0]).all()
            assert np.hypot(far[:, 0] - FAR_TRUE[0], far[:, 1] - FAR_TRUE[1]).max() < 0.5


# ---- 9. R = 15 is match_ncc_full_chip_planes, in both modes, on a 12-bit and on an 8-bit pair ----
@pytest.mark.parametrize("ocw", [16, 10])
@pytest.mark.parametrize("bits", [12, 8])
def test_r15_is_full_chip_planes(api, ocw, bits):
    c, i0, i1, shift = fu.u8_case(ocw, 15)
    if bits == 12:
        i0, i1 = spread12(i0), spread12(i1)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for mode in (0, 1):
            for npeaks in (0, 4):
                want = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, 15, npeaks, shift=shift, mode=mode, surface=True)
                path = ctx.last_path()
                got = ctx.match_ncc_wide_planes(c.xyuvav, c.offset, ocw, 15, npeaks, shift=shift, mode=mode, surface=True)
                assert ctx.last_path() == path
                assert path == (wp.CHIP_PATH if mode == 1 else {(12, 16): "u16_full", (12, 10): wp.CHIP_PATH, (8, 16): "u8_mfma_full", (8, 10): "u8_mfma_chip"}[bits, ocw])
                assert same_bytes(got, want)


# ---- 10. the mode-0 dispatch, last_path after every call ----
def other_class(kind, i0, i1):
    if kind == "dn12":
        return spread12(i0), spread12(i1)
    if kind == "dn16":
        return to_dn16(i0, 21), to_dn16(i1, 22)
    return to_float(i0, 23), to_float(i1, 24)


def test_mode0_on_an_8bit_pair_goes_where_wide_class_sends_it(api):
    import wide_u8_common as wu
    for ocw in (16, 10):
        f = wu.fixture(ocw, 24, ocw == 10, True, 0)
        with api.Context(0) as ctx:
            ctx.set_images(f["i0"], f["i1"])
            for npeaks in (0, 4):
                want = ctx.match_ncc_wide_class(f["xy"], f["off"], ocw, 24, npeaks, shift=f["shift"], swap=f["swap"], mode=0, surface=True)
                assert ctx.last_path() == wp.U8_PATH
                got = run(ctx, f, npeaks, mode=0, path=wp.U8_PATH)
                assert same_bytes(got, want)


@pytest.mark.parametrize("ocw,radius", [(16, 24), (10, 24), (40, 45)])
def test_mode0_on_a_12bit_pair(api, ocw, radius):
    """inside the float wide kernel's range (16, 24) the measured rule names the matrix-core kernel, with match_ncc_wide's bytes; outside
    it -- another chip size (10, 24), a radius beyond its limit at ocw 40 (39) -- the matrix-core kernel is the only one"""
    f = wp.fixture(ocw, radius, "dn12", False, True)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in (0, 4):
            a = run(ctx, f, npeaks, mode=0)
            b = run(ctx, f, npeaks, mode=1)
            assert same_bytes(a, b)
            if (ocw, radius) == (16, 24):
                vs_wide(ctx, f, a, npeaks, f"mode 0, npeaks {npeaks}")
            else:
                with pytest.raises(api.Mimc3Error):                         # (the float wide kernel does not take it)
                    ctx.match_ncc_wide(f["xy"], f["off"], ocw, radius, npeaks, shift=f["shift"])


@pytest.mark.parametrize("kind", ["dn16", "float"])
def test_mode0_on_wider_classes(api, kind):
    """at ocw 16, R 24 the bytes and the path of match_ncc_wide; at ocw 10 refused with MIMC3_EUNSUPPORTED; mode 1 refused"""
    import wide_u8_common as wu
    f = wu.fixture(16, 24, False, True, 0)
    j0, j1 = other_class(kind, f["i0"], f["i1"])
    with api.Context(0) as ctx:
        ctx.set_images(j0, j1)
        for npeaks in (0, 4):
            want = ctx.match_ncc_wide(f["xy"], f["off"], 16, 24, npeaks, shift=f["shift"], surface=True)
            assert ctx.last_path() == wp.FLOAT_PATH
            got = run(ctx, f, npeaks, mode=0, path=wp.FLOAT_PATH)
            assert same_bytes(got, want)
        for ocw, mode in ((10, 0), (16, 1), (10, 1)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_wide_planes(f["xy"], f["off"], ocw, 24, 0, shift=f["shift"], mode=mode)
            assert e.value.code == -6, (ocw, mode)
            assert ctx.last_path() == wp.FLOAT_PATH                         # (a refusal leaves last_path alone)


# ---- 11. refusals, each against untouched output buffers ----
def test_refusals(api):
    f = wp.fixture(16, 24, "dn12", False, True)
    n = f["xy"].shape[0]
    xy, off, sh = np.array(f["xy"]), np.array(f["off"]), np.array(f["shift"])
    call = api._lib.mimc3_match_ncc_wide_planes

    def refused(ctx, ocw, radius, mode, npeaks, with_cand, code, why):
        out = np.full((n, 8), 7.5, np.float32)
        surf = np.full((n, 95 * 95), 7.5, np.float32)
        cand = np.full((8, n, 3), 7.5, np.float32)
        rc = call(ctx._h, xy, n, off, sh.ctypes.data, ocw, radius, npeaks, 0, mode, out, cand.ctypes.data if with_cand else None, surf.ctypes.data)
        assert rc == code, f"{why}: rc {rc}"
        assert (out == 7.5).all() and (surf == 7.5).all() and (cand == 7.5).all(), why + ": an output buffer was written"

    with api.Context(0) as ctx:
        refused(ctx, 16, 24, 1, 0, False, -5, "no images")                  # MIMC3_ESTATE
        ctx.set_images(f["i0"], f["i1"])
        for ocw, radius, mode, npeaks, with_cand, why in ((0, 24, 0, 0, False, "ocw 0"), (81, 24, 1, 0, False, "ocw 81"), (16, 48, 0, 0, False, "R 48"),
                                                          (16, 48, 1, 0, False, "R 48, mode 1"), (10, 0, 1, 0, False, "R 0"), (80, 48, 1, 0, False, "ocw 80 R 48"),
                                                          (16, 24, 2, 0, False, "mode 2"), (16, 24, -1, 0, False, "mode -1"),
                                                          (16, 24, 0, 4, False, "npeaks without cand"), (16, 24, 1, 0, True, "cand without npeaks"),
                                                          (16, 24, 1, 9, True, "npeaks 9")):
            refused(ctx, ocw, radius, mode, npeaks, with_cand, -1, why)
        # beyond the kernel's radius at a chip size the float wide kernel does not take: MIMC3_EUNSUPPORTED, the limit in the message
        for ocw, radius in ((80, 28), (80, 47), (73, 35), (69, 47)):
            for mode in (0, 1):
                refused(ctx, ocw, radius, mode, 0, False, -6, f"ocw {ocw} R {radius} mode {mode}")
                msg = api._lib.mimc3_last_error().decode()
                assert "mimc3_wide_planes_max_radius" in msg and str(api.wide_planes_max_radius(ocw)) in msg, msg
        sh[3] = (4000, 0)                                                   # a search box that leaves the zero border: MIMC3_EBOUNDS
        refused(ctx, 16, 24, 1, 0, False, -2, "bounds")
        refused(ctx, 16, 24, 0, 0, False, -2, "bounds, mode 0")


# ---- 12. the _dev entry, one point outside the image and one box outside the zero border ----
def test_dev_entry_and_a_point_outside_the_image(api):
    import hipmem
    from hipmem import DevArray
    ocw, radius, npeaks = 10, 24, 4
    f = wp.fixture(ocw, radius, "dn12", True, True)
    n = f["xy"].shape[0]
    xy, shift = np.array(f["xy"]), np.array(f["shift"])
    xy[3, 2] = ocw - 1                                                  # the chip leaves the image: only the _dev entry passes it
    shift[5] = (4000, 0)                                                # the box leaves the zero border
    bad = [3, 5]
    S2 = (2 * radius + 1) ** 2
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        d_xy, d_sh = DevArray(src=xy), DevArray(src=shift)
        d_out, d_cand, d_surf = DevArray((n, 8), np.float32), DevArray((npeaks, n, 3), np.float32), DevArray((n, S2), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_wide_planes_dev(d_xy.ptr, n, f["off"], ocw, radius, npeaks, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr,
                                      stream=st.value, swap=True, mode=1, d_surf=d_surf.ptr)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == wp.PATH
        out, cand, surf = run(ctx, f, npeaks)
        good = np.setdiff1d(np.arange(n), bad)
        got_out, got_cand, got_surf = d_out.numpy(), d_cand.numpy(), d_surf.numpy()
        assert_bits_equal(got_out[good], out[good], "_dev: record")
        assert_bits_equal(got_cand[:, good], cand[:, good], "_dev: candidates")
        assert_bits_equal(got_surf[good], surf[good], "_dev: surface")
        assert np.isnan(got_out[bad]).all() and np.isnan(got_cand[:, bad]).all() and np.isnan(got_surf[bad]).all()
        with pytest.raises(api.Mimc3Error) as e:                        # the host entry refuses both points
            ctx.match_ncc_wide_planes(xy, f["off"], ocw, radius, npeaks, shift=shift, swap=True, mode=1)
        assert e.value.code == -2
        assert hipmem._hip.hipStreamDestroy(st) == 0


# ---- 13. downstream: the surfaces are a layer of a wide stack ----
def test_surfaces_are_stack_layers(api):
    f = wp.fixture(16, 24, "dn12", False, True)
    n, npeaks = f["xy"].shape[0], 4
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        rec, cand, surf = run(ctx, f, npeaks)
        ctx.stack_begin_wide(n, 24, f["shift"])
        ctx.stack_add_surfaces(surf, rec[:, 2] == -3)
        a = ctx.stack_finish(npeaks, 1)
        ctx.stack_begin_wide(n, 24, f["shift"])
        ctx.stack_add(f["xy"], f["off"], 16)
        b = ctx.stack_finish(npeaks, 1)
        ctx.stack_begin(0, 0)
    for x, y, name in zip(a, b, ("record", "candidates", "count")):
        assert x.tobytes() == y.tobytes(), "stack_add_surfaces vs stack_add: " + name
