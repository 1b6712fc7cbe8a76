"""GPU: the exhaustive search on scaled-integer pairs (12-bit DN, filtered 8-bit pairs) at any chip half-width 1..80 on the matrix cores
(mimc3_match_ncc_full_chip_planes, match_full_chip_u16_kernel.hip).

Unless a case says otherwise it compares record, candidates and surface byte for byte with match_ncc_full_chip(mode=1, surface=True) --
the run-time-ocw float kernel, whose sums are the same exact integers (times a power of two) on such pixels -- at npeaks 0 and 4, and
asserts the path "u16_mfma_chip".  A subset is also held against the CPU oracle of tests/full_any_common.py directly: the surface bit
for bit, record and candidates the oracle's tail of the device surface.  The fixtures are those of tests/full_chip_u16_common.py
(tests/test_full_chip_u16_cpu.py counts them): 12 points -- 6 clean, 2 with a null in the box only, 2 in the chip only, 2 on both sides
-- every non-null pixel spread over all twelve bits.  The chip sizes come from the library's own layout query."""
import ctypes as C

import numpy as np
import pytest

import full_chip_common as fc
import full_chip_u8_common as fu
import full_chip_u16_common as fp
from conftest import assert_bits_equal
from full_any_common import full_any, tail_from_surface
from full_multi_common import STATUS_R

pytestmark = pytest.mark.gpu
NPEAKS = (0, 4)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check(ctx, xy, off, ocw, radius, shift, swap, what, npeaks_list=NPEAKS, mode=1, oracle_pair=None, path=fp.PATH):
    """The new entry against match_ncc_full_chip(mode 1) and, given the float pair, against the oracle -> (record, surface)"""
    rec = surf = None
    for npeaks in npeaks_list:
        ref = ctx.match_ncc_full_chip(xy, off, ocw, radius, npeaks, shift=shift, swap=swap, mode=1, surface=True)
        assert ctx.last_path() == fc.PATH
        got = ctx.match_ncc_full_chip_planes(xy, off, ocw, radius, npeaks, shift=shift, swap=swap, mode=mode, surface=True)
        assert ctx.last_path() == path
        tag = f"{what}, npeaks {npeaks}"
        assert_bits_equal(got[2], ref[2], tag + ": surface vs match_ncc_full_chip(mode 1)")
        assert_bits_equal(got[0], ref[0], tag + ": record vs match_ncc_full_chip(mode 1)")
        if npeaks:
            assert_bits_equal(got[1], ref[1], tag + ": candidates vs match_ncc_full_chip(mode 1)")
        else:
            assert got[1] is None
        if oracle_pair is not None:
            want_rec, _, want_surf, _ = full_any(oracle_pair[0], oracle_pair[1], xy, off, ocw, radius, 0, shift=shift, swap=swap)
            st3 = want_rec[:, 2] == -3
            assert_bits_equal(got[2], want_surf, tag + ": surface vs the oracle")
            assert np.isnan(got[2][st3]).all() and np.array_equal(got[0][:, 2] == -3, st3)
            t_rec, t_cand = tail_from_surface(got[2], shift, radius, npeaks, refused=st3, device_snr_order=True)
            assert_bits_equal(got[0], t_rec, tag + ": record vs the tail of the device surface")
            if npeaks:
                assert_bits_equal(got[1], t_cand, tag + ": candidates vs the tail of the device surface")
        bare = ctx.match_ncc_full_chip_planes(xy, off, ocw, radius, npeaks, shift=shift, swap=swap, mode=mode)        # without surfaces
        assert ctx.last_path() == path
        assert_bits_equal(bare[0], got[0], tag + ": record without surfaces")
        if npeaks:
            assert_bits_equal(bare[1], got[1], tag + ": candidates without surfaces")
        rec, surf = got[0], got[2]
    return rec, surf


def run_fixture(api, ocw, radius, kind="dn12", nulls="placed", swap=False, with_shift=True, oracle=False, npeaks_list=NPEAKS):
    c, i0, i1, shift = fp.u16_case(ocw, radius, kind, nulls, swap, with_shift)
    sgn = -1 if swap else 1
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, surf = check(ctx, c.xyuvav, sgn * c.offset, ocw, radius, None if shift is None else sgn * shift, swap,
                          f"ocw {ocw} R {radius} {kind} {nulls} swap {swap} shift {with_shift}", npeaks_list,
                          oracle_pair=(i0, i1) if oracle else None)
    return c, rec, surf


# ---- 1. the chip sizes: the layout's boundaries from the library's own query ----
def test_size_cases_are_the_librarys(api):
    assert fp.size_cases(api.full_chip_planes_layout) == fp.size_cases()
    assert fp.boundaries(api.full_chip_planes_layout)["KCW"] == [(24, 25), (56, 57)]


@pytest.mark.parametrize("ocw,radius", fp.size_cases())
def test_chip_sizes(api, ocw, radius):
    c, rec, surf = run_fixture(api, ocw, radius, oracle=True)           # (12 points: the oracle stays under a second at every size)
    assert (rec[:, 2] >= -1).any() and np.isfinite(surf).all()
    for g in fp.BOX_ONLY + fp.CHIP_ONLY + fp.BOTH:
        assert rec[g, 2] >= -1 or rec[g, 2] == -4


# ---- 2. radius, direction, shift ----
@pytest.mark.parametrize("ocw,radius", fp.RADII)
def test_radii(api, ocw, radius):
    run_fixture(api, ocw, radius)


@pytest.mark.parametrize("ocw,swap,with_shift", [(10, True, True), (57, True, True), (10, False, False), (10, True, False)])
def test_direction_and_shift(api, ocw, swap, with_shift):
    run_fixture(api, ocw, 7 if ocw == 10 else 15, swap=swap, with_shift=with_shift, oracle=ocw == 10)


# ---- 3. the null patterns ----
@pytest.mark.parametrize("ocw", [10, 60])
def test_null_free_pair_and_all_points_dirty(api, ocw):
    run_fixture(api, ocw, 7, nulls="none")                              # the masked launch finds no point
    run_fixture(api, ocw, 7, nulls="all", oracle=True)                  # the clean launch finishes none


# ---- 4. saturated 12-bit pairs: the table cut (44 | 45) and the finish's rounding products (75 | 76, 80) ----
@pytest.mark.parametrize("ocw", fp.SATURATED_OCW)
@pytest.mark.parametrize("kind", ["sat3", "sat63"])
def test_saturated_pairs(api, ocw, kind):
    run_fixture(api, ocw, 15, kind=kind, oracle=ocw in (45, 76))


# ---- 5. scale 8 on both images and on one ----
@pytest.mark.parametrize("ocw", [10, 60])
@pytest.mark.parametrize("kind", ["eighths", "mixed"])
def test_eighths_and_the_mixed_scale(api, ocw, kind):
    run_fixture(api, ocw, 7, kind=kind, oracle=ocw == 10)


# ---- 6. the filtered forms of an 8-bit pair ----
@pytest.mark.parametrize("ocw", [10, 57])
@pytest.mark.parametrize("which", [0, 2], ids=["ddx", "laplacian"])
def test_filtered_pairs(api, ocw, which):
    radius = 7
    c, i0, i1, shift = fu.u8_case(ocw, radius)
    with api.Context(0) as ctx:
        f0, f1 = fp.filtered_pair(ctx, api, which, i0, i1)
        check(ctx, c.xyuvav, c.offset, ocw, radius, shift, False, f"filter {which} ocw {ocw}", oracle_pair=(f0, f1) if ocw == 10 else None)
        a = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, radius, 4, shift=shift, surface=True)          # mode 0: the same kernel
        b = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, radius, 4, shift=shift, mode=1, surface=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 7. mode 1 at each of the six; an 8-bit pair; mode 0's dispatch ----
@pytest.mark.parametrize("ocw", fp.SIX)
def test_mode1_at_the_six_is_full_surf(api, ocw):
    radius = fp.six_radius(ocw)
    c, i0, i1, shift = fp.u16_case(ocw, radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check(ctx, c.xyuvav, c.offset, ocw, radius, shift, False, f"ocw {ocw} R {radius}")
        for npeaks in NPEAKS:
            want = ctx.match_ncc_full_surf(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift)
            assert ctx.last_path() == "u16_full"
            got = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift, mode=1, surface=True)
            assert ctx.last_path() == fp.PATH
            for a, b, name in zip(got, want, ("record", "candidates", "surface")):
                if npeaks or name != "candidates":
                    assert_bits_equal(a, b, f"ocw {ocw} npeaks {npeaks}: {name} vs match_ncc_full_surf")
            pl = ctx.match_ncc_full_planes(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift)
            assert_bits_equal(got[0], pl[0], f"ocw {ocw} npeaks {npeaks}: record vs match_ncc_full_planes")
            if npeaks:
                assert_bits_equal(got[1], pl[1], f"ocw {ocw} npeaks {npeaks}: candidates vs match_ncc_full_planes")


@pytest.mark.parametrize("ocw", [10, 16, 60])
def test_mode1_on_an_8bit_pair_is_the_u8_kernels_bytes(api, ocw):
    c, i0, i1, shift = fu.u8_case(ocw, 7)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in NPEAKS:
            want = ctx.match_ncc_full_chip_class(c.xyuvav, c.offset, ocw, 7, npeaks, shift=shift, mode=1, surface=True)
            assert ctx.last_path() == fu.PATH
            got = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, 7, npeaks, shift=shift, mode=1, surface=True)
            assert ctx.last_path() == fp.PATH
            assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(got, want))
        if ocw != 16:                                                   # mode 0 on an 8-bit pair outside the six: the u8 kernel
            got = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, 7, 4, shift=shift, surface=True)
            assert ctx.last_path() == fu.PATH
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_mode0_at_16_is_the_class_dispatch(api):
    c, i0, i1, shift = fp.u16_case(16, 7)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in NPEAKS:
            want = ctx.match_ncc_full_chip_class(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift, surface=True)
            assert ctx.last_path() == "u16_full"
            got = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift, surface=True)
            assert ctx.last_path() == "u16_full"
            assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(got, want))
            bare = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift)
            assert ctx.last_path() == "u16_full"
            ref = ctx.match_ncc_full_chip(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift)
            assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(bare, ref))
        a = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, 10, 7, 4, shift=shift, surface=True)    # mode 0 at another chip size
        assert ctx.last_path() == fp.PATH
        b = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, 10, 7, 4, shift=shift, mode=1, surface=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["u16", "float"])
def test_mode0_on_other_classes_is_the_float_kernel(api, kind):
    c, i0, i1, shift = fc.chip_case(kind, 10, 7)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in NPEAKS:
            want = ctx.match_ncc_full_chip(c.xyuvav, c.offset, 10, 7, npeaks, shift=shift, surface=True)
            assert ctx.last_path() == fc.PATH
            got = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, 10, 7, npeaks, shift=shift, surface=True)
            assert ctx.last_path() == fc.PATH
            assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(got, want))


# ---- 8. statuses ----
@pytest.mark.parametrize("ocw", [10, 64])
def test_statuses(api, ocw):
    j0, j1, xy, shift = fc.chip_status_case(ocw)
    i0, i1 = fp.spread12(j0, by_position=False), fp.spread12(j1, by_position=False)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, surf = check(ctx, xy, (0, 0), ocw, STATUS_R, shift, False, f"statuses ocw {ocw}", oracle_pair=(i0, i1))
        out, cand = ctx.match_ncc_full_chip_planes(xy, (0, 0), ocw, STATUS_R, 4, shift=shift, mode=1)
    st = rec[:, 2]
    assert st[0] == -3 and np.isnan(surf[0]).all() and np.isnan(rec[0, [0, 1, 3, 4, 5, 6, 7]]).all()
    assert (cand[:, 0, 2] == -3).all() and np.isnan(cand[:, 0, :2]).all()
    assert st[1] == -2 and not np.isfinite(surf[1]).any() and (cand[:, 1, 2] == -2).all()
    assert st[2] == -4 and (cand[:, 2, 2] >= -1).any()


def test_dev_entry_and_a_point_outside_the_image(api):
    import hipmem
    from hipmem import DevArray
    ocw, radius, npeaks = 10, 7, 4
    c, i0, i1, shift = fp.u16_case(ocw, radius)
    xy = np.array(c.xyuvav, np.float64)
    xy[3, 2] = ocw - 1                                                  # the chip leaves the image: only the _dev entry passes it
    shift = np.array(shift, np.int32)
    shift[5] = (1000, 0)                                                # the box leaves the zero border
    bad = [3, 5]
    S2 = (2 * radius + 1) ** 2
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        d_xy, d_sh = DevArray(src=xy), DevArray(src=shift)
        d_out, d_cand, d_surf = DevArray((c.n, 8), np.float32), DevArray((npeaks, c.n, 3), np.float32), DevArray((c.n, S2), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_full_chip_planes_dev(d_xy.ptr, c.n, c.offset, ocw, radius, npeaks, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr,
                                           stream=st.value, mode=1, d_surf=d_surf.ptr)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == fp.PATH
        good = np.setdiff1d(np.arange(c.n), bad)
        out, cand, surf = ctx.match_ncc_full_chip(xy[good], c.offset, ocw, radius, npeaks, shift=shift[good], mode=1, surface=True)
        got_out, got_cand, got_surf = d_out.numpy(), d_cand.numpy(), d_surf.numpy()
        assert_bits_equal(got_out[good], out, "_dev: record")
        assert_bits_equal(got_cand[:, good], cand, "_dev: candidates")
        assert_bits_equal(got_surf[good], surf, "_dev: surface")
        assert np.isnan(got_out[bad]).all() and np.isnan(got_cand[:, bad]).all() and np.isnan(got_surf[bad]).all()
        with pytest.raises(api.Mimc3Error) as e:                        # the host entry refuses both points
            ctx.match_ncc_full_chip_planes(xy, c.offset, ocw, radius, npeaks, shift=shift, mode=1)
        assert e.value.code == -2
        assert hipmem._hip.hipStreamDestroy(st) == 0


# ---- 9. refusals, each against untouched output buffers ----
def test_refusals(api):
    c, i0, i1, shift = fp.u16_case(10, 7)
    n = c.n
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    off = np.ascontiguousarray(c.offset, np.int32)
    sh = np.ascontiguousarray(shift, np.int32)
    call = api._lib.mimc3_match_ncc_full_chip_planes

    def refused(ctx, ocw, radius, mode, npeaks, with_cand, code, why):
        out = np.full((n, 8), 7.5, np.float32)
        surf = np.full((n, 31 * 31), 7.5, np.float32)
        cand = np.full((8, n, 3), 7.5, np.float32)
        rc = call(ctx._h, xy, n, off, sh.ctypes.data, ocw, radius, npeaks, 0, mode, out, cand.ctypes.data if with_cand else None, surf.ctypes.data)
        assert rc == code, f"{why}: rc {rc}"
        assert (out == 7.5).all() and (surf == 7.5).all() and (cand == 7.5).all(), why + ": an output buffer was written"

    def bad_args(ctx, why, code=-1, **kw):
        """one argument of a good call replaced: a null context, point array or record, N <= 0; a point whose chip leaves the image"""
        out = np.full((n, 8), 7.5, np.float32)
        surf = np.full((n, 31 * 31), 7.5, np.float32)
        a = dict(handle=ctx._h, xy=xy.ctypes.data, n=n, out=out.ctypes.data, sh=sh.ctypes.data)
        a.update(kw)
        raw = C.CDLL(api._lib._name).mimc3_match_ncc_full_chip_planes   # (a handle of its own, without argtypes: a null pointer can be passed)

        def p_(v):
            return v if isinstance(v, C.c_void_p) else C.c_void_p(v)
        rc = raw(p_(a["handle"]), p_(a["xy"]), C.c_int32(a["n"]), p_(off.ctypes.data), p_(a["sh"]), C.c_int32(10), C.c_int32(7),
                 C.c_int32(0), C.c_int32(0), C.c_int32(1), p_(a["out"]), p_(None), p_(surf.ctypes.data))
        assert rc == code, f"{why}: rc {rc}"
        assert (out == 7.5).all() and (surf == 7.5).all(), why + ": an output buffer was written"

    with api.Context(0) as ctx:
        refused(ctx, 10, 7, 1, 0, False, -5, "no images")               # MIMC3_ESTATE
        ctx.set_images(i0, i1)
        bad_args(ctx, "null context", handle=None)
        bad_args(ctx, "null point array", xy=None)
        bad_args(ctx, "null record", out=None)
        bad_args(ctx, "N 0", n=0)
        bad_args(ctx, "N -1", n=-1)
        outside = xy.copy()
        outside[3, 2] = 10 - 1                                          # the chip leaves the image
        bad_args(ctx, "a chip outside the image", code=-2, xy=outside.ctypes.data)      # MIMC3_EBOUNDS
        far = sh.copy()
        far[5] = (1000, 0)                                              # the search box leaves the zero border
        bad_args(ctx, "a box outside the zero border", code=-2, sh=far.ctypes.data)
        for ocw, radius, mode, npeaks, with_cand, why in ((0, 7, 0, 0, False, "ocw 0"), (81, 7, 0, 0, False, "ocw 81"), (0, 7, 1, 0, False, "ocw 0, mode 1"),
                                                          (81, 7, 1, 0, False, "ocw 81, mode 1"), (10, 16, 0, 0, False, "R 16"), (10, 16, 1, 0, False, "R 16, mode 1"),
                                                          (10, 0, 1, 0, False, "R 0"), (10, 7, 2, 0, False, "mode 2"), (10, 7, -1, 0, False, "mode -1"),
                                                          (10, 7, 0, 4, False, "npeaks without cand"),
                                                          (10, 7, 1, 0, True, "cand without npeaks"), (10, 7, 1, 9, True, "npeaks 9")):
            refused(ctx, ocw, radius, mode, npeaks, with_cand, -1, why)
            if ocw in (0, 81):
                assert "1..80" in api._lib.mimc3_last_error().decode()
        rec = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, 10, 7, 0, shift=shift, mode=1)[0]
        assert ctx.last_path() == fp.PATH and (rec[:, 2] >= -1).any()
    for kind in ("u16", "float"):                                       # mode 1 takes 8-bit and scaled-integer pairs only
        k, j0, j1, _ = fc.chip_case(kind, 10, 7)
        with api.Context(0) as ctx:
            ctx.set_images(j0, j1)
            xy, n = np.ascontiguousarray(k.xyuvav, np.float64), k.n
            sh = np.zeros((n, 2), np.int32)
            refused(ctx, 10, 7, 1, 0, False, -6, f"mode 1 on a {kind} pair")       # MIMC3_EUNSUPPORTED
            assert "scaled-integer" in api._lib.mimc3_last_error().decode()
            refused(ctx, 10, 7, 2, 0, False, -1, f"mode 2 on a {kind} pair")


# ---- 10. downstream: a surface at ocw 10 is a stack layer ----
def test_surfaces_are_stack_layers(api):
    ocw, radius, npeaks = 10, 7, 4
    c, i0, i1, shift = fp.u16_case(ocw, radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, cand, surf = ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift, surface=True)
        assert ctx.last_path() == fp.PATH
        ctx.stack_begin(c.n, radius, shift)
        ctx.stack_add_surfaces(surf, rec[:, 2] == -3)
        s_rec, s_cand, count = ctx.stack_finish(npeaks, 1)
        ctx.stack_begin(0, 0)
    assert_bits_equal(s_rec, rec, "stack of one layer: record")
    assert_bits_equal(s_cand, cand, "stack of one layer: candidates")
    assert (count == (rec[:, 2] != -3)).all()


# ---- 11. full_candidates over the reference's other chip set, default variants: the calls made by hand ----
def test_full_candidates_any_ocw(api):
    vec_ocw, radius, npeaks = (7, 10, 15, 11), 7, 2
    c, i0, i1, shift = fu.u8_case(10, radius)
    variants = (None,) + tuple(api.CLI_KERNELS)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        dp = ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, radius, npeaks, shift=shift, any_ocw=True)
        assert dp.shape == (len(variants) * len(vec_ocw) * npeaks, c.n, 3)
        b = 0
        for k in variants:
            ctx.filter_images(None)
            if k is not None:
                ctx.filter_images(k)
            for ocw in vec_ocw:
                want = ctx.match_ncc_full_chip(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift, mode=1)[1]
                assert_bits_equal(dp[npeaks * b:npeaks * (b + 1)], want, f"variant {b // len(vec_ocw)} ocw {ocw}")
                if ocw not in fp.SIX:
                    ctx.match_ncc_full_chip_planes(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift)
                    assert ctx.last_path() == (fu.PATH if k is None else fp.PATH)
                b += 1
        ctx.filter_images(None)
