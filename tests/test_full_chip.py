"""GPU: the exhaustive search at any chip half-width 1..80 (mimc3_match_ncc_full_chip, match_full_chip_kernel.hip).

Against the oracle of tests/full_any_common.py, whose definition takes any chip size: the surface's finite mask is the oracle's; on
8-bit, 16-bit and float_case pairs every f64 sum is exact in any order, so the surface is the reference-order oracle's bit for bit
whatever the bands and bodies; on the six-decade wide_case pair every finite cell is within 1 f32 ulp (tests/test_full_chip_cpu.py
shows that the oracle's own two orders meet that on these fixtures); record and candidates are the oracle's tail of the DEVICE surface
bit for bit.  The chip sizes: 1, 2, 3 (a chip row of less than two 4-pixel chunks), 10 and 11 (both paddings of a chip row), the
band-boundary sizes derived from full_chip_band_rows (full_chip_common.band_shape_cases: at R 15 the band rule has only the one-band
shape, the others come at the largest R that has them), and 64 and 80 at R 15 (the LDS ceiling) and R 1."""
import ctypes as C

import numpy as np
import pytest

import full_chip_common as fc
from conftest import assert_bits_equal
from full_any_common import full_any, surface_distance, tail_from_surface
from full_multi_common import STATUS_R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check(ctx, i0, i1, xy, off, ocw, radius, shift, swap, exact, what, npeaks_list=(0, 4)):
    """mode 1 of the resident pair against the oracle -> (record, surface)"""
    want_rec, _, want_surf, _ = full_any(i0, i1, xy, off, ocw, radius, 0, shift=shift, swap=swap)
    rec, none, surf = ctx.match_ncc_full_chip(xy, off, ocw, radius, 0, shift=shift, swap=swap, mode=1, surface=True)
    assert none is None and ctx.last_path() == fc.PATH
    st3 = want_rec[:, 2] == -3
    assert np.array_equal(rec[:, 2] == -3, st3), what + ": status -3 points"
    assert_bits_equal(rec[st3], want_rec[st3], what + ": status -3 records")
    assert np.isnan(surf[st3]).all()
    share, worst = surface_distance(surf, want_surf, what)              # (asserts that the finite masks are equal)
    print(f"{what}: {share:.6f} of the finite cells differ from the oracle, at most {worst} ulp")
    if exact:
        assert_bits_equal(surf, want_surf, what + ": surface vs the oracle (exact sums)")
    else:
        assert worst <= 1, f"{what}: a cell {worst} ulp from the oracle"
    for npeaks in npeaks_list:
        out, cand = ctx.match_ncc_full_chip(xy, off, ocw, radius, npeaks, shift=shift, swap=swap, mode=1)
        assert ctx.last_path() == fc.PATH
        t_rec, t_cand = tail_from_surface(surf, shift, radius, npeaks, refused=st3, device_snr_order=True)
        assert_bits_equal(out, t_rec, what + f": record vs the tail of the device surface, npeaks {npeaks}")
        if npeaks:
            assert_bits_equal(cand, t_cand, what + f": candidates vs the tail of the device surface, npeaks {npeaks}")
        else:
            assert cand is None
            assert_bits_equal(out, rec, what + ": the record again")
    return rec, surf


def run_fixture(api, kind, ocw, radius, enc, swap, npeaks_list=(0, 4)):
    c, i0, i1, shift = fc.chip_case(kind, ocw, radius, enc)
    sgn = -1 if swap else 1
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, surf = check(ctx, i0, i1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap, fc.EXACT[kind],
                          f"{kind} ocw {ocw} R {radius} {enc} swap {swap}", npeaks_list)
    return c, i0, i1, shift, rec, surf


# ---- 1. the small chips, every kind, both ways round ----
@pytest.mark.parametrize("kind,ocw,radius,enc,swap", fc.small_fixtures())
def test_small_chips(api, kind, ocw, radius, enc, swap):
    run_fixture(api, kind, ocw, radius, enc, swap, npeaks_list=(0, 1, 8))


# ---- 2. every radius (few tasks: the rows of a task dealt to lanes), the three encodings ----
@pytest.mark.parametrize("kind,ocw,radius,enc,swap", fc.radius_fixtures())
def test_radii(api, kind, ocw, radius, enc, swap):
    run_fixture(api, kind, ocw, radius, enc, swap)


def test_without_shift_and_without_nulls(api):
    c, i0, i1, shift = fc.chip_case("wide", 10, 15)
    clean0, clean1 = np.where(i0 == 0, np.float32(3), i0), np.where(i1 == 0, np.float32(3), i1)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check(ctx, i0, i1, c.xyuvav, c.offset + np.array([3, -2], np.int32), 10, 15, None, False, False, "wide ocw 10 no shift")
        ctx.set_images(clean0, clean1)
        check(ctx, clean0, clean1, c.xyuvav, c.offset, 10, 15, shift, False, False, "wide ocw 10 no nulls")


# ---- 3. the band boundaries and the LDS ceiling ----
@pytest.mark.parametrize("kind,ocw,radius,enc,swap", fc.band_fixtures())
def test_bands(api, kind, ocw, radius, enc, swap):
    # the shapes come from the library's own band heights: the Python rule that listed the cases must be the library's
    assert api.full_chip_band_rows(ocw, radius) == fc.band_rows(ocw, radius)
    cases = fc.band_shape_cases(api.full_chip_band_rows)
    assert cases == fc.band_shape_cases() and set(cases) == set(fc.BAND_SHAPES)
    c, i0, i1, shift, rec, surf = run_fixture(api, kind, ocw, radius, enc, swap)
    bands = fc.band_classes(i0, i1, c.xyuvav, c.offset, shift, ocw, radius, rows=api.full_chip_band_rows)
    clean, dirty, mixed = fc.class_counts(bands)
    assert clean >= 3 and dirty >= 3
    if len(bands[0]) > 1:
        # mixed bands: a dirty point with a band without an excluded pixel; a point whose only null sits in the last box row / column
        last_row, last_col = fc.only_null_in_last_box_line(i1, c.xyuvav, c.offset, shift, ocw, radius)
        assert mixed >= 1 and last_row and last_col
        for g in last_row + last_col:
            assert np.isfinite(surf[g]).all() and (rec[g, 2] >= -1 or rec[g, 2] == -4)     # (at R 1 the peak may sit on the border)


# ---- 4. mode 1 at three of the six built chip sizes IS the float kernel's result ----
@pytest.mark.parametrize("kind,ocw,radius,enc,swap", fc.mode1_fixtures())
def test_mode1_equals_full_any_mode1(api, kind, ocw, radius, enc, swap):
    c, i0, i1, shift = fc.chip_case(kind, ocw, radius, enc)
    what = f"{kind} ocw {ocw} R {radius}"
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in (0, 4):
            want = ctx.match_ncc_full_any(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift, mode=1, surface=True)
            assert ctx.last_path() == "f32g_full"
            got = ctx.match_ncc_full_chip(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift, mode=1, surface=True)
            assert ctx.last_path() == fc.PATH
            if fc.EXACT[kind]:
                assert_bits_equal(got[2], want[2], what + ": surface vs match_ncc_full_any(mode 1)")
                assert_bits_equal(got[0], want[0], what + ": record vs match_ncc_full_any(mode 1)")
                if npeaks:
                    assert_bits_equal(got[1], want[1], what + ": candidates vs match_ncc_full_any(mode 1)")
            else:
                share, worst = surface_distance(got[2], want[2], what)
                print(f"{what}: {share:.6f} of the finite cells differ from match_ncc_full_any(mode 1), at most {worst} ulp")
                assert worst <= 1


# ---- 5. mode 0 at one of the six IS match_ncc_full_any(mode 0) ----
def test_mode0_at_a_built_size_is_full_any(api):
    c, i0, i1, shift = fc.chip_case("u8", 16, 7)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in (0, 4):
            want = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift)
            assert ctx.last_path() == "u8_mfma_full"
            got = ctx.match_ncc_full_chip(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift)
            assert ctx.last_path() == "u8_mfma_full"
            assert got[0].tobytes() == want[0].tobytes()
            assert (got[1] is None and want[1] is None) or got[1].tobytes() == want[1].tobytes()
        # mode 0 at another chip size on the same 8-bit pair: the new kernel, and mode 1's bytes
        a = ctx.match_ncc_full_chip(c.xyuvav, c.offset, 10, 7, 4, shift=shift, surface=True)
        assert ctx.last_path() == fc.PATH
        b = ctx.match_ncc_full_chip(c.xyuvav, c.offset, 10, 7, 4, shift=shift, mode=1, surface=True)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


# ---- 6. statuses ----
@pytest.mark.parametrize("ocw", [10, 64])
def test_statuses(api, ocw):
    i0, i1, xy, shift = fc.chip_status_case(ocw)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, surf = check(ctx, i0, i1, xy, (0, 0), ocw, STATUS_R, shift, False, True, f"statuses ocw {ocw}")
        out, cand = ctx.match_ncc_full_chip(xy, (0, 0), ocw, STATUS_R, 4, shift=shift, mode=1)
    st = rec[:, 2]
    assert st[0] == -3 and np.isnan(surf[0]).all() and np.isnan(rec[0, [0, 1, 3, 4, 5, 6, 7]]).all()
    assert (cand[:, 0, 2] == -3).all() and np.isnan(cand[:, 0, :2]).all()
    assert st[1] == -2 and not np.isfinite(surf[1]).any() and (cand[:, 1, 2] == -2).all()
    assert st[2] == -4 and (cand[:, 2, 2] >= -1).any()                  # the interior candidates that exist
    assert (st[3:6] != -3).all() and st[6] >= -1


def test_dev_entry_and_a_point_outside_the_image(api):
    import hipmem
    from hipmem import DevArray
    ocw, radius, npeaks = 10, 7, 4
    c, i0, i1, shift = fc.chip_case("wide", ocw, radius, "nan_zero")
    xy = np.ascontiguousarray(c.xyuvav)
    xy[3, 2] = ocw - 1                                                  # the chip leaves the image: only the _dev entry passes it
    shift = np.ascontiguousarray(shift, np.int32)
    shift[5] = (1000, 0)                                                # the box leaves the zero border
    bad = [3, 5]
    S2 = (2 * radius + 1) ** 2
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        d_xy, d_sh = DevArray(src=xy), DevArray(src=shift)
        d_out, d_cand, d_surf = DevArray((c.n, 8), np.float32), DevArray((npeaks, c.n, 3), np.float32), DevArray((c.n, S2), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_full_chip_dev(d_xy.ptr, c.n, c.offset, ocw, radius, npeaks, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, stream=st.value,
                                    mode=1, d_surf=d_surf.ptr)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == fc.PATH
        good = np.setdiff1d(np.arange(c.n), bad)
        out, cand, surf = ctx.match_ncc_full_chip(xy[good], c.offset, ocw, radius, npeaks, shift=shift[good], mode=1, surface=True)
        got_out, got_cand, got_surf = d_out.numpy(), d_cand.numpy(), d_surf.numpy()
        assert_bits_equal(got_out[good], out, "_dev: record")
        assert_bits_equal(got_cand[:, good], cand, "_dev: candidates")
        assert_bits_equal(got_surf[good], surf, "_dev: surface")
        assert np.isnan(got_out[bad]).all() and np.isnan(got_cand[:, bad]).all() and np.isnan(got_surf[bad]).all()
        with pytest.raises(api.Mimc3Error) as e:                        # the host entry refuses both points
            ctx.match_ncc_full_chip(xy, c.offset, ocw, radius, npeaks, shift=shift, mode=1)
        assert e.value.code == -2
        assert hipmem._hip.hipStreamDestroy(st) == 0


# ---- 7. refusals, each against an untouched output buffer ----
def test_refusals(api):
    c, i0, i1, shift = fc.chip_case("u8", 16, 7)
    n = c.n
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    off = np.ascontiguousarray(c.offset, np.int32)
    sh = np.ascontiguousarray(shift, np.int32)
    call = api._lib.mimc3_match_ncc_full_chip
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for ocw, radius, mode, with_surf, why in ((0, 7, 0, False, "ocw 0"), (81, 7, 0, False, "ocw 81"), (0, 7, 1, False, "ocw 0, mode 1"),
                                                  (81, 7, 1, False, "ocw 81, mode 1"), (10, 16, 0, False, "R 16"), (10, 0, 1, False, "R 0"),
                                                  (10, 7, 2, False, "mode 2"), (10, 7, -1, False, "mode -1"),
                                                  (16, 7, 0, True, "surf at mode 0, ocw 16, 8-bit pair")):
            out = np.full((n, 8), 7.5, np.float32)
            surf = np.full((n, 225), 7.5, np.float32)
            rc = call(ctx._h, xy, n, off, sh.ctypes.data, ocw, radius, 0, 0, mode, out, None, surf.ctypes.data if with_surf else None)
            assert rc == -1, why
            assert (out == 7.5).all() and (surf == 7.5).all(), why + ": an output buffer was written"
            if ocw in (0, 81):
                assert "1..80" in api._lib.mimc3_last_error().decode()
        # the older entries keep the six
        for older in (ctx.match_ncc_full_any, ctx.match_ncc_full_dn):
            with pytest.raises(api.Mimc3Error) as e:
                older(c.xyuvav, c.offset, 10, 7, 0, shift=shift)
            assert e.value.code == -1 and "7, 15, 16, 30, 32, 40" in str(e.value)
        rec = ctx.match_ncc_full_chip(c.xyuvav, c.offset, 10, 7, 0, shift=shift)[0]
        assert ctx.last_path() == fc.PATH and (rec[:, 2] >= -1).any()


# ---- 8. downstream: a surface from an arbitrary chip size is a stack layer ----
def test_surfaces_are_stack_layers(api):
    ocw, radius, npeaks = 10, 7, 4
    c, i0, i1, shift = fc.chip_case("u8", ocw, radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, cand, surf = ctx.match_ncc_full_chip(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift, surface=True)
        assert ctx.last_path() == fc.PATH
        ctx.stack_begin(c.n, radius, shift)
        ctx.stack_add_surfaces(surf, rec[:, 2] == -3)
        s_rec, s_cand, count = ctx.stack_finish(npeaks, 1)
        ctx.stack_begin(0, 0)
    assert_bits_equal(s_rec, rec, "stack of one layer: record")
    assert_bits_equal(s_cand, cand, "stack of one layer: candidates")
    assert (count == (rec[:, 2] != -3)).all()


# ---- 9. full_candidates over the reference's other chip set ----
def test_full_candidates_any_ocw(api):
    vec_ocw, radius, npeaks = (7, 10, 15, 11), 7, 2
    c, i0, i1, shift = fc.chip_case("u8", 10, radius)
    kernels = (None, api.CLI_KERNELS[2])
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        with pytest.raises(ValueError):                                 # ndp = 10 x 4 x 2 = 80 > 64: refused before any device work
            ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, radius, npeaks, kernels=(None,) * 10, shift=shift, any_ocw=True)
        with pytest.raises(api.Mimc3Error) as e:                        # the default keeps today's calls
            ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, radius, npeaks, kernels=kernels, shift=shift)
        assert e.value.code == -1
        dp = ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, radius, npeaks, kernels=kernels, shift=shift, any_ocw=True)
        assert dp.shape == (len(kernels) * len(vec_ocw) * npeaks, c.n, 3) and dp.dtype == np.float32
        b = 0
        for k in kernels:
            ctx.filter_images(None)
            ctx.filter_images(k)
            for ocw in vec_ocw:
                want = ctx.match_ncc_full_chip(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift)[1]
                assert (ctx.last_path() == fc.PATH) == (ocw in (10, 11))
                assert_bits_equal(dp[b:b + npeaks], want, f"block (variant {k is not None}, ocw {ocw})")
                b += npeaks
        ctx.filter_images(None)
        assert (dp[:, :, 2] >= -1).mean() > 0.5
