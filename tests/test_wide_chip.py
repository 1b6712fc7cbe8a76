"""GPU: the exhaustive search beyond +-15 px on ANY pair at any chip half-width 1..80 (mimc3_match_ncc_wide_chip,
match_wide_chip_kernel.hip).

Everywhere the oracle of tests/full_any_common.py judges (wide_chip_common.judge): on 8-, 12- and 16-bit pairs the surface bit for bit, a
non-finite cell of the same kind; on float pairs every finite cell within 1 f32 ulp; record and candidates equal the oracle's tail of the
DEVICE surface bit for bit on every pair.  The fixtures are those of tests/wide_chip_common.py (tests/test_wide_chip_cpu.py qualifies
them): points whose boxes do not overlap -- one null in the last box row, one in the last box column, one in the first chip row, nulls on
both sides, one a column outside the box, one inside a single tile's window, a -4 in the last partial tile, a -3 by each rule."""
import ctypes as C

import numpy as np
import pytest

import full_chip_u8_common as fu
import wide_chip_common as wc
from conftest import assert_bits_equal
from full_any_common import full_any
from full_chip_common import BAND_SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def run(ctx, f, pts, npeaks, mode=1, surface=True, path=wc.PATH):
    xy, sh = wc.sub(f, pts)
    got = ctx.match_ncc_wide_chip(xy, f["off"], f["ocw"], f["R"], npeaks, shift=sh, swap=f["swap"], mode=mode, surface=surface)
    assert ctx.last_path() == path
    return got


def check_fixture(api, fx, peaks=(0, 4)):
    f = wc.fixture(*fx)
    pts, o_rec, o_surf = wc.oracle(*fx)
    xy, sh = wc.sub(f, pts)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in peaks:
            got = run(ctx, f, pts, npeaks)
            what = f"{f['what']}, npeaks {npeaks}"
            wc.judge(got, o_rec, o_surf, sh, f["R"], npeaks, f["exact"], what)
            bare = run(ctx, f, pts, npeaks, surface=False)
            assert_bits_equal(bare[0], got[0], what + ": record without surfaces")
            if npeaks:
                assert_bits_equal(bare[1], got[1], what + ": candidates without surfaces")
    rec = got[0]
    assert rec[pts.index(wc.G4), 2] == -4 and rec[pts.index(wc.G3CHIP), 2] == -3
    return pts, got


def ids(fx):
    return "-".join(str(x) for x in fx)


# ---- 1. tile edges: S = 33 (a second tile of one cell), 63, 65 (three tiles, the last of one cell), 95; with and without shift, swapped ----
@pytest.mark.parametrize("fx", wc.TILE_EDGES, ids=ids)
def test_tile_edges(api, fx):
    check_fixture(api, fx, peaks=(0, 1, 8) if fx[1] == 16 else (0, 4))


# ---- 2. band shapes from the library's own layout, the largest chip at both ends of the range, the smallest chip ----
def test_band_shapes_come_from_the_library(api):
    found = wc.band_shape_cases(api.wide_chip_layout)
    assert found == wc.band_shape_cases(wc.layout) and set(found) == set(BAND_SHAPES) - {"full_last_band"}


@pytest.mark.parametrize("fx", wc.band_fixtures(), ids=ids)
def test_band_shapes(api, fx):
    assert fx in wc.band_fixtures(api.wide_chip_layout)
    check_fixture(api, fx, peaks=(0, 4) if fx[0] < 70 else (4,))


# ---- 3. bodies: the placed nulls are judged above on 16-bit pairs; here float pixels with -9999 / NaN nulls and the six-decade pair ----
@pytest.mark.parametrize("fx", wc.BODIES, ids=ids)
def test_bodies_on_float_pairs(api, fx):
    pts, got = check_fixture(api, fx)
    rec, surf = got[0], got[2]
    for g in wc.BOX_ONLY + wc.CHIP_ONLY + wc.BOTH + (wc.OUTSIDE, wc.ONE_TILE):
        assert np.isfinite(surf[pts.index(g)]).all() and rec[pts.index(g), 2] >= -1


def test_placed_nulls_are_finished_points(api):
    pts, got = check_fixture(api, wc.TILE_EDGES[2], peaks=(0,))
    for g in wc.BOX_ONLY + wc.CHIP_ONLY + wc.BOTH + (wc.OUTSIDE, wc.ONE_TILE):
        assert np.isfinite(got[2][pts.index(g)]).all()


# ---- 4. statuses at R 32, three tiles per axis ----
def test_statuses(api):
    pts, got = check_fixture(api, wc.STATUS, peaks=(0, 4))
    st = got[0][:, 2]
    assert st[wc.G4] == -4 and st[wc.G3CHIP] == -3 and st[wc.G3BOX] == -3 and st[wc.ONE_TILE] == -2
    assert st[wc.CLEAN] != -3 and np.isfinite(got[2][wc.CLEAN]).any()           # the 60 % box is searched


# ---- 5. a box flush with the planes' 256-px border ----
def test_box_flush_with_the_border(api):
    ocw, R = 10, 16
    f = wc.fixture(ocw, R, "u16", False, True, "zero", False)
    H, W = f["i0"].shape
    h = ocw + R
    xy = np.ascontiguousarray(f["xy"][[0, 11, 9, 4]])
    off = f["off"]
    sh = np.zeros((4, 2), np.int32)
    sh[0] = (-256 + h - int(xy[0, 2]) - int(off[0]), -256 + h - int(xy[0, 3]) - int(off[1]))              # left and top
    sh[1] = (W + 255 - h - int(xy[1, 2]) - int(off[0]), H + 255 - h - int(xy[1, 3]) - int(off[1]))        # right and bottom
    sh[2:] = f["shift"][[9, 4]]
    o_rec, _, o_surf, _ = full_any(f["i0"], f["i1"], xy, off, ocw, R, 0, shift=sh)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in (0, 4):
            got = ctx.match_ncc_wide_chip(xy, off, ocw, R, npeaks, shift=sh, mode=1, surface=True)
            assert ctx.last_path() == wc.PATH
            wc.judge(got, o_rec, o_surf, sh, R, npeaks, True, f"flush boxes, npeaks {npeaks}")
        for g, d in ((0, (-1, 0)), (0, (0, -1)), (1, (1, 0)), (1, (0, 1))):     # one pixel further: the host entry refuses
            bad = sh.copy()
            bad[g] += d
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_wide_chip(xy, off, ocw, R, 0, shift=bad, mode=1)
            assert e.value.code == -2
    assert got[0][0, 2] == -3 and got[0][1, 2] == -3 and np.isfinite(got[0][2:, 0]).all()


# ---- 6. equal bytes with the siblings ----
@pytest.mark.parametrize("fx", [(16, 24, "u16"), (40, 39, "u16"), (16, 24, "u8"), (40, 39, "u8")], ids=ids)
def test_mode1_at_the_six_is_match_ncc_wide(api, fx):
    ocw, R, kind = fx
    full = (ocw, R, kind, False, True, "zero", False)
    f = wc.fixture(*full)
    pts, o_rec, o_surf = wc.oracle(*full)
    xy, sh = wc.sub(f, pts)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in (0, 4):
            got = run(ctx, f, pts, npeaks)
            what = f"{f['what']}, npeaks {npeaks}"
            wc.judge(got, o_rec, o_surf, sh, R, npeaks, True, what)
            ref = ctx.match_ncc_wide(xy, f["off"], ocw, R, npeaks, shift=sh, surface=True)
            assert ctx.last_path() == wc.FLOAT_PATH
            wc.same_surface(got[2], ref[2], what + ": surface vs match_ncc_wide")
            assert_bits_equal(got[0], ref[0], what + ": record vs match_ncc_wide")
            if npeaks:
                assert_bits_equal(got[1], ref[1], what + ": candidates vs match_ncc_wide")


@pytest.mark.parametrize("kind", ["u8", "dn12"])
def test_mode1_outside_the_six_is_the_class_kernels_bytes(api, kind):
    ocw, R = 10, 20
    f = wc.fixture(ocw, R, kind, False, True, "zero", False)
    pts = wc.points(ocw)
    xy, sh = wc.sub(f, pts)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        for npeaks in (0, 4):
            sib = ctx.match_ncc_wide_class if kind == "u8" else ctx.match_ncc_wide_planes
            want = sib(xy, f["off"], ocw, R, npeaks, shift=sh, mode=1, surface=True)
            assert ctx.last_path() == (wc.U8_PATH if kind == "u8" else wc.U16_PATH)
            got = run(ctx, f, pts, npeaks)
            what = f"{f['what']}, npeaks {npeaks}"
            wc.same_surface(got[2], want[2], what + ": surface vs the class kernel")
            assert_bits_equal(got[0], want[0], what + ": record vs the class kernel")
            if npeaks:
                assert_bits_equal(got[1], want[1], what + ": candidates vs the class kernel")


CLS = ("u8", "dn12", "u16", "float")                    # one pair of every class, in the order of mimc3_wide_chip_path's pair_class
R15_NAMES = {6: "u8_mfma_full", 7: "u16_full", 8: "f32i_full", 9: "f32g_full", 11: "f32g_chip", 12: "u8_mfma_chip", 13: "u16_mfma_chip"}


@pytest.mark.parametrize("ocw", [16, 10])
@pytest.mark.parametrize("kind", CLS)
def test_r15_is_the_table(api, ocw, kind):
    """R 15: mode 1 is match_ncc_full_chip(mode 1) (path 11), mode 0 is match_ncc_full_chip_planes(mode 0): kernel, bytes, last_path"""
    c, b0, b1, shift = fu.u8_case(ocw, 15)
    i0, i1 = wc._map(b0, kind, 21), wc._map(b1, kind, 22)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for mode in (0, 1):
            for npeaks in (0, 4):
                sib = ctx.match_ncc_full_chip if mode == 1 else ctx.match_ncc_full_chip_planes
                want = sib(c.xyuvav, c.offset, ocw, 15, npeaks, shift=shift, mode=mode, surface=True)
                path = ctx.last_path()
                got = ctx.match_ncc_wide_chip(c.xyuvav, c.offset, ocw, 15, npeaks, shift=shift, mode=mode, surface=True)
                assert ctx.last_path() == path
                assert path == R15_NAMES[api.wide_chip_path(CLS.index(kind), ocw, 15, mode)] and (mode == 0 or path == wc.CHIP_PATH)
                assert same_bytes(got, want), (ocw, kind, mode, npeaks)


# ---- 7. the mode-0 dispatch, last_path after every call ----
NAMES = {10: wc.FLOAT_PATH, 14: wc.U8_PATH, 15: wc.U16_PATH, 16: wc.PATH}


@pytest.mark.parametrize("ocw,R", [(16, 24), (10, 24), (40, 45), (80, 30)])
@pytest.mark.parametrize("kind", CLS)
def test_mode0_dispatch(api, ocw, R, kind):
    f = wc.fixture(ocw, R, kind, False, True, "zero", False)
    pts = wc.points(ocw)
    xy, sh = wc.sub(f, pts)
    want_path = api.wide_chip_path(CLS.index(kind), ocw, R, 0)
    assert want_path == wc.path(CLS.index(kind), ocw, R, 0, api.wide_planes_max_radius)
    if (ocw, R, kind) == (80, 30, "dn12"):
        assert R > api.wide_planes_max_radius(ocw) and want_path == 16
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        npeaks = 4
        got = run(ctx, f, pts, npeaks, mode=0, path=NAMES[want_path])
        ref = run(ctx, f, pts, npeaks, mode=1)
        what = f"{f['what']}: mode 0 on {NAMES[want_path]} vs mode 1"
        if f["exact"] or want_path == 16:       # (exact sums: every kernel's bytes; path 16: the same kernel in both modes)
            wc.same_surface(got[2], ref[2], what)
            assert_bits_equal(got[0], ref[0], what + ": record")
            assert_bits_equal(got[1], ref[1], what + ": candidates")
        sib = {10: lambda: ctx.match_ncc_wide(xy, f["off"], ocw, R, npeaks, shift=sh, surface=True),
               14: lambda: ctx.match_ncc_wide_class(xy, f["off"], ocw, R, npeaks, shift=sh, mode=0, surface=True),
               15: lambda: ctx.match_ncc_wide_planes(xy, f["off"], ocw, R, npeaks, shift=sh, mode=0, surface=True)}.get(want_path)
        if sib:
            want = sib()
            assert ctx.last_path() == NAMES[want_path]
            assert same_bytes(got, want), what + ": the sibling's bytes"
        else:                                   # no other entry takes the call
            for other in (ctx.match_ncc_wide_planes, ctx.match_ncc_wide_class):
                with pytest.raises(api.Mimc3Error) as e:
                    other(xy, f["off"], ocw, R, npeaks, shift=sh, mode=0)
                assert e.value.code == -6


# ---- 8. refusals, each against untouched output buffers ----
def test_refusals(api):
    f = wc.fixture(10, 24, "u16", False, True, "zero", False)
    n = f["xy"].shape[0]
    xy, off, sh = np.array(f["xy"]), np.array(f["off"]), np.array(f["shift"])
    call = api._lib.mimc3_match_ncc_wide_chip

    def refused(ctx, ocw, radius, mode, npeaks, with_cand, code, why):
        out = np.full((n, 8), 7.5, np.float32)
        surf = np.full((n, 95 * 95), 7.5, np.float32)
        cand = np.full((8, n, 3), 7.5, np.float32)
        before = ctx.last_path()
        rc = call(ctx._h, xy, n, off, sh.ctypes.data, ocw, radius, npeaks, 0, mode, out, cand.ctypes.data if with_cand else None, surf.ctypes.data)
        assert rc == code, f"{why}: rc {rc}"
        assert (out == 7.5).all() and (surf == 7.5).all() and (cand == 7.5).all(), why + ": an output buffer was written"
        assert ctx.last_path() == before, why + ": last_path moved"

    with api.Context(0) as ctx:
        refused(ctx, 10, 24, 1, 0, False, -5, "no images")                  # MIMC3_ESTATE
        refused(ctx, 10, 24, 0, 0, False, -5, "no images, mode 0")
        ctx.set_images(f["i0"], f["i1"])
        for ocw, radius, mode, npeaks, with_cand, why in ((0, 24, 0, 0, False, "ocw 0"), (81, 24, 1, 0, False, "ocw 81"), (10, 0, 1, 0, False, "R 0"),
                                                          (10, 48, 0, 0, False, "R 48"), (80, 48, 1, 0, False, "ocw 80 R 48"), (10, 24, 2, 0, False, "mode 2"),
                                                          (10, 24, -1, 0, False, "mode -1"), (10, 24, 0, 4, False, "npeaks without cand"),
                                                          (10, 24, 1, 0, True, "cand without npeaks"), (10, 24, 1, 9, True, "npeaks 9")):
            refused(ctx, ocw, radius, mode, npeaks, with_cand, -1, why)
        sh[3] = (4000, 0)                                                   # a search box that leaves the zero border: MIMC3_EBOUNDS
        refused(ctx, 10, 24, 1, 0, False, -2, "bounds")
        refused(ctx, 10, 24, 0, 0, False, -2, "bounds, mode 0")
        xy[5, 2] = 9                                                        # a chip that leaves the image
        sh[3] = 0
        refused(ctx, 10, 24, 1, 0, False, -2, "chip bounds")


# ---- 9. the _dev entry on its own stream, one point outside the image and one box outside the zero border ----
def test_dev_entry_and_a_point_outside_the_image(api):
    import hipmem
    from hipmem import DevArray
    ocw, radius, npeaks = 10, 24, 4
    f = wc.fixture(ocw, radius, "u16", False, True, "zero", False)
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
        ctx.match_ncc_wide_chip_dev(d_xy.ptr, n, f["off"], ocw, radius, npeaks, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr,
                                    stream=st.value, mode=1, d_surf=d_surf.ptr)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == wc.PATH
        out, cand, surf = run(ctx, f, range(n), npeaks)
        good = np.setdiff1d(np.arange(n), bad)
        got_out, got_cand, got_surf = d_out.numpy(), d_cand.numpy(), d_surf.numpy()
        assert_bits_equal(got_out[good], out[good], "_dev: record")
        assert_bits_equal(got_cand[:, good], cand[:, good], "_dev: candidates")
        assert_bits_equal(got_surf[good], surf[good], "_dev: surface")
        assert np.isnan(got_out[bad]).all() and np.isnan(got_cand[:, bad]).all() and np.isnan(got_surf[bad]).all()
        with pytest.raises(api.Mimc3Error) as e:                        # the host entry refuses both points
            ctx.match_ncc_wide_chip(xy, f["off"], ocw, radius, npeaks, shift=shift, mode=1)
        assert e.value.code == -2
        assert hipmem._hip.hipStreamDestroy(st) == 0


# ---- 10. downstream: the surfaces are a layer of a wide stack ----
def test_surfaces_are_a_stack_layer(api):
    ocw, R, npeaks = 10, 20, 4
    f = wc.fixture(ocw, R, "u16", False, True, "zero", False)
    n = f["xy"].shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        rec, cand, surf = run(ctx, f, range(n), npeaks)
        ctx.stack_begin_wide(n, R, f["shift"])
        ctx.stack_add_surfaces(surf, rec[:, 2] == -3)
        s_rec, s_cand, s_count = ctx.stack_finish(npeaks, 1)
        ctx.stack_begin(0, 0)
    assert_bits_equal(s_rec, rec, "the stack of one layer: record")
    assert_bits_equal(s_cand, cand, "the stack of one layer: candidates")
    assert np.array_equal(s_count, (rec[:, 2] != -3).astype(np.uint16))


# ---- 11. full_candidates beyond R 15 at any chip size ----
def test_full_candidates_beyond_15(api):
    R, npeaks, ocws = 20, 2, (10, 16)
    f = wc.fixture(16, R, "u16", False, True, "zero", False)
    pts = (0, 2, 4, 6, 9)
    xy, sh = wc.sub(f, pts)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        dp = ctx.full_candidates(xy, f["off"], ocws, R, npeaks, kernels=(None,), shift=sh, any_ocw=True)
        blocks = []
        for ocw, path in zip(ocws, (wc.PATH, wc.FLOAT_PATH)):
            blocks.append(ctx.match_ncc_wide_chip(xy, f["off"], ocw, R, npeaks, shift=sh, mode=0)[1])
            assert ctx.last_path() == path
        assert dp.shape == (len(ocws) * npeaks, len(pts), 3)
        assert_bits_equal(dp, np.concatenate(blocks, axis=0), "full_candidates(any_ocw, radius 20) vs the single calls")
        # (radius <= 15 runs exactly the calls it ran before)
        dp15 = ctx.full_candidates(xy, f["off"], ocws, 15, npeaks, kernels=(None,), shift=sh, any_ocw=True)
        want = [ctx.match_ncc_full_chip_planes(xy, f["off"], 10, 15, npeaks, shift=sh)[1], ctx.match_ncc_full_chip(xy, f["off"], 16, 15, npeaks, shift=sh)[1]]
        assert_bits_equal(dp15, np.concatenate(want, axis=0), "full_candidates(any_ocw, radius 15)")
