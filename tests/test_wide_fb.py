"""GPU: forward-backward consistency beyond +-15 px (mimc3_match_ncc_wide_fb).

The entry's record, candidates and fb rows equal, bit for bit (NaNs by position), fb_chain (tests/full_fb_common.py) driven by
Context.match_ncc_wide itself -- two ordinary calls with the seed and compose arithmetic on the host -- on one pair per pixel class, with
and without a per-point shift; at R 15 the bytes are match_ncc_full_fb(mode=1)'s; on the pair displaced by (34, -27) px at R 40 the fb
rows equal the chain and the err of the correctly matched points is printed; refusals; the _dev entry on a stream of its own."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_fb_common import FB_OFFSET, class_pair, fb_chain, fb_points
from wide_common import FAR_OCW, FAR_R, FAR_TRUE, far_case

pytestmark = pytest.mark.gpu

WIDE, FULL = "f32g_wide", "f32g_full"
SHAPES = ((7, 16, (0, 3)), (16, 24, (2,)))          # (ocw, R, the npeaks checked)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def wide_search(ctx):
    """Context.match_ncc_wide with match_ncc_full_any's signature (the wide entry is mode 1 by definition)"""
    def search(xy, offset, ocw, radius, npeaks, shift=None, swap=False, mode=0):
        return ctx.match_ncc_wide(xy, offset, ocw, radius, npeaks, shift=shift, swap=swap)
    return search


def check_chain(ctx, xy, offset, ocw, radius, npeaks, shift, H, W, what):
    out, cand, fb = ctx.match_ncc_wide_fb(xy, offset, ocw, radius, npeaks, shift=shift)
    assert ctx.last_path() == (WIDE if radius >= 16 else FULL), what + ": last_path reports the forward path"
    n = xy.shape[0]
    assert out.shape == (n, 8) and fb.shape == (1 + npeaks, n, 4) and (cand is None) == (npeaks == 0)
    w_out, w_cand, w_fb, why = fb_chain(wide_search(ctx), xy, offset, ocw, radius, H, W, npeaks=npeaks, shift=shift)
    assert_bits_equal(out, w_out, what + ": record")
    if npeaks:
        assert_bits_equal(cand, w_cand, what + ": candidates")
    assert_bits_equal(fb, w_fb, what + ": fb")
    return out, fb, why


@pytest.mark.parametrize("ocw,radius,peaks", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ("u8", "dn12", "dn16", "float"))
def test_equals_the_chain_of_wide_calls(api, kind, ocw, radius, peaks):
    i0, i1, _ = class_pair(kind)
    H, W = i0.shape
    xy, shift = fb_points(ocw=ocw, radius=radius)
    rows = np.zeros(7, np.int64)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in peaks:
            for sh in (shift, None):
                what = f"{kind} ocw {ocw} R {radius} npeaks {npeaks} shift {sh is not None}"
                out, fb, why = check_chain(ctx, xy, FB_OFFSET, ocw, radius, npeaks, sh, H, W, what)
                rows += np.bincount(why.ravel(), minlength=7)
                assert (fb[:, :, 2][why == 5] == -5).all() and (fb[:, :, 2][why == 6] == -6).all()
                fit = fb[0, :, 2] >= -1
                assert fit.any()
                if npeaks:
                    assert_bits_equal(fb[1][fit], fb[0][fit], "plane 1 vs plane 0 where the record has a fit")
        check_chain(ctx, xy[:1], FB_OFFSET, ocw, radius, peaks[-1], shift[:1], H, W, f"{kind} ocw {ocw} R {radius}: N = 1")
    # the fixture holds rows of every kind (counted on the host, from the seed's reasons): searched, -5 and -6
    print(f"{kind} ocw {ocw} R {radius}: rows searched {rows[0]}, -5 {rows[5]}, -6 {rows[6]}")
    assert rows[0] >= 40 and rows[5] >= 1 and rows[6] >= 1


@pytest.mark.parametrize("kind", ("u8", "float"))
def test_r15_is_match_ncc_full_fb_mode_1(api, kind):
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=16, radius=15)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in (0, 3):
            want = ctx.match_ncc_full_fb(xy, FB_OFFSET, 16, 15, npeaks, shift=shift, mode=1)
            got = ctx.match_ncc_wide_fb(xy, FB_OFFSET, 16, 15, npeaks, shift=shift)
            assert ctx.last_path() == FULL
            for a, b, name in zip(got, want, ("record", "candidates", "fb")):
                if b is None:
                    assert a is None
                else:
                    assert a.tobytes() == b.tobytes(), f"{kind} R 15, npeaks {npeaks}: {name}"
    assert (want[2][0, :, 2] >= -1).sum() >= 20


def test_far_pair_at_r40(api):
    """What it is for: the pair displaced by (34, -27) px.  The fb rows are the chain's; the err of the correctly matched points is
    printed (README: forward-backward beyond 15 px), no threshold is asserted."""
    c = far_case()
    H, W = c.i0.shape
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        out, fb, why = check_chain(ctx, c.xyuvav, (0, 0), FAR_OCW, FAR_R, 3, None, H, W, "far pair, R 40, npeaks 3")
    good = np.isfinite(out[:, 0]) & (np.hypot(out[:, 0] - FAR_TRUE[0], out[:, 1] - FAR_TRUE[1]) < 0.5)
    err = fb[0, good, 3]
    print(f"far pair R 40: {int(good.sum())} of {out.shape[0]} points matched within 0.5 px; backward rows searched {int((why[0] == 0).sum())}; "
          f"err of the matched points min {np.nanmin(err):.4f} median {np.nanmedian(err):.4f} max {np.nanmax(err):.4f} px, "
          f"not finite {int((~np.isfinite(err)).sum())}")
    with np.errstate(invalid="ignore"):
        rest = fb[1:, :, 3][np.isfinite(fb[1:, :, 3]) & (fb[1:, :, 3] != fb[0, :, 3][None, :])]
    if rest.size:
        print(f"far pair R 40: err of the {rest.size} other candidates with a backward fit min {rest.min():.3f} median {np.median(rest):.3f} px")
    assert good.all()                                       # (tests/test_wide.py: the wide search fits every point of this pair)


def test_refusals(api):
    i0, i1, _ = class_pair("u8")
    xy, shift = fb_points(ocw=7, radius=16)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        out, fb, cand = np.empty((n, 8), np.float32), np.empty((10, n, 4), np.float32), np.empty((9, n, 3), np.float32)
        off = np.ascontiguousarray(FB_OFFSET)
        call = api._lib.mimc3_match_ncc_wide_fb
        assert call(ctx._h, xy, n, off, None, 7, 16, 0, out, None, fb.ctypes.data) == -5                  # no images: MIMC3_ESTATE
        ctx.set_images(i0, i1)
        assert call(ctx._h, xy, n, off, None, 7, 16, 0, out, None, None) == -1                            # fb NULL
        assert call(ctx._h, xy, n, off, None, 7, 16, 9, out, cand.ctypes.data, fb.ctypes.data) == -1      # npeaks 9
        assert call(ctx._h, xy, n, off, None, 7, 16, 2, out, None, fb.ctypes.data) == -1                  # cand / npeaks mismatch
        assert call(ctx._h, xy, n, off, None, 8, 16, 0, out, None, fb.ctypes.data) == -1                  # ocw 8
        for ocw in (7, 40):
            assert call(ctx._h, xy, n, off, None, ocw, api.wide_max_radius(ocw) + 1, 0, out, None, fb.ctypes.data) == -1
        assert call(ctx._h, xy, n, off, None, 7, 0, 0, out, None, fb.ctypes.data) == -1
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_wide_fb(xy, (300, 0), 7, 16, 0)                                                  # the forward box leaves the border
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_fb(xy, FB_OFFSET, 7, 16, 0)                                                 # the old entry keeps its range
        assert e.value.code == -1
        a = ctx.match_ncc_wide_fb(xy, FB_OFFSET, 7, 16, 1, shift=shift)
        b = ctx.match_ncc_wide_fb(xy, FB_OFFSET, 7, 16, 1, shift=shift)
        assert ctx.last_path() == WIDE
        for x, y, what in zip(a, b, ("record", "candidates", "fb")):
            assert_bits_equal(x, y, "two identical calls after the refusals: " + what)


def test_dev_entry_on_a_stream(api):
    import hipmem
    from hipmem import DevArray
    i0, i1, _ = class_pair("dn16")
    ocw, R = 16, 20
    xy, shift = fb_points(ocw=ocw, radius=R)
    calls = ((7, 1), (60, 3), (7, 1), (60, 0))                     # (N, npeaks): the scratch grows, is reused, and serves fewer rows
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        want = {k: ctx.match_ncc_wide_fb(xy[:k[0]], FB_OFFSET, ocw, R, k[1], shift=shift[:k[0]]) for k in set(calls)}
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        d_xy, d_sh = DevArray(src=xy), DevArray(src=shift)
        got = []
        for n, npeaks in calls:                                    # (a fresh pair: the first call builds the planes itself)
            d_out, d_fb = DevArray((n, 8), np.float32), DevArray((1 + npeaks, n, 4), np.float32)
            d_cand = DevArray((npeaks, n, 3), np.float32) if npeaks else None
            ctx.match_ncc_wide_fb_dev(d_xy.ptr, n, FB_OFFSET, ocw, R, npeaks, d_out.ptr, d_fb.ptr, d_cand=d_cand.ptr if npeaks else 0,
                                      d_shift=d_sh.ptr, stream=st.value)
            got.append((d_out, d_cand, d_fb))
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == WIDE
        for (n, npeaks), (d_out, d_cand, d_fb) in zip(calls, got):
            w_out, w_cand, w_fb = want[(n, npeaks)]
            assert_bits_equal(d_out.numpy(), w_out, f"_dev N {n} npeaks {npeaks}: record")
            assert_bits_equal(d_fb.numpy(), w_fb, f"_dev N {n} npeaks {npeaks}: fb")
            if npeaks:
                assert_bits_equal(d_cand.numpy(), w_cand, f"_dev N {n} npeaks {npeaks}: candidates")
        assert hipmem._hip.hipStreamDestroy(st) == 0
