"""GPU: the forward-backward consistency check (mimc3_match_ncc_full_fb, fb_kernel.hip).

The entry's record, candidates and fb rows equal, bit for bit (NaNs by position), fb_chain (tests/full_fb_common.py) driven by
Context.match_ncc_full_any itself -- two ordinary calls through the existing entries with the seed and compose arithmetic on the host --
on one pair per pixel class and in mode 1; on the 8-bit fixture of tests/test_full_fb_cpu.py the fb rows equal the C-oracle chain's,
so the three statuses are seen on the device; the forward bytes are those of match_ncc_full_any alone, before and after; the _dev
entry on a stream of its own returns the host entry's bytes while its scratch grows and is reused."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_fb_common import FB_OCW, FB_OFFSET, FB_R, class_pair, fb_chain, fb_pair, fb_points, oracle_search

pytestmark = pytest.mark.gpu

SHAPES = ((7, 4), (16, 15), (40, 6))
NPEAKS = (0, 1, 3, 8)
KINDS = (("u8", 0), ("dn12", 0), ("dn16", 0), ("float", 0), ("u8", 1))


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_chain(ctx, xy, ocw, radius, npeaks, shift, mode, path, H, W, what):
    out, cand, fb = ctx.match_ncc_full_fb(xy, FB_OFFSET, ocw, radius, npeaks, shift=shift, mode=mode)
    assert ctx.last_path() == path, what + ": last_path reports the forward path"
    n = xy.shape[0]
    assert out.shape == (n, 8) and fb.shape == (1 + npeaks, n, 4) and (cand is None) == (npeaks == 0)
    w_out, w_cand, w_fb, why = fb_chain(ctx.match_ncc_full_any, xy, FB_OFFSET, ocw, radius, H, W, npeaks=npeaks, shift=shift, mode=mode)
    assert_bits_equal(out, w_out, what + ": record")
    if npeaks:
        assert_bits_equal(cand, w_cand, what + ": candidates")
    assert_bits_equal(fb, w_fb, what + ": fb")
    return fb, why


@pytest.mark.parametrize("ocw,radius", SHAPES)
@pytest.mark.parametrize("kind,mode", KINDS)
def test_equals_the_chain_of_ordinary_calls(api, kind, mode, ocw, radius):
    i0, i1, path = class_pair(kind)
    if mode == 1:
        path = "f32g_full"
    H, W = i0.shape
    xy, shift = fb_points(ocw=ocw, radius=radius)
    seen = set()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in NPEAKS:
            for sh in (shift, None):
                fb, why = check_chain(ctx, xy, ocw, radius, npeaks, sh, mode, path, H, W,
                                      f"{kind} mode {mode} ocw {ocw} R {radius} npeaks {npeaks} shift {sh is not None}")
                seen |= set(np.unique(why).tolist())
                fit = fb[0, :, 2] >= -1
                assert fit.any()
                if npeaks:
                    assert_bits_equal(fb[1][fit], fb[0][fit], "plane 1 vs plane 0 where the record has a fit")
        # one point alone (and a grid of one block's worth is not needed: 60 is no multiple of 64)
        check_chain(ctx, xy[:1], ocw, radius, 3, shift[:1], mode, path, H, W, f"{kind} mode {mode} ocw {ocw} R {radius}: N = 1")
        check_chain(ctx, xy[57:58], ocw, radius, 0, None, mode, path, H, W, f"{kind} mode {mode} ocw {ocw} R {radius}: N = 1, nothing searched")
    assert seen == {0, 5, 6}, seen


def test_the_cpu_fixture_equals_the_oracle_chain(api):
    """The 8-bit fixture of tests/test_full_fb_cpu.py: the matrix-core record's (du, dv) and the candidates are the C oracle's bit for
    bit, so the whole fb array is the oracle chain's -- with the statuses -5, -6 and a passed-through -4."""
    i0, i1 = fb_pair()
    H, W = i0.shape
    xy, shift = fb_points()
    _, w_cand, w_fb, _ = fb_chain(oracle_search(i0, i1), xy, FB_OFFSET, FB_OCW, FB_R, H, W, npeaks=3, shift=shift)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand, fb = ctx.match_ncc_full_fb(xy, FB_OFFSET, FB_OCW, FB_R, 3, shift=shift)
        assert ctx.last_path() == "u8_mfma_full"
    assert_bits_equal(cand, w_cand, "candidates vs the oracle")
    assert_bits_equal(fb, w_fb, "fb vs the oracle chain")
    st = fb[0, :, 2]
    assert st[56] == -5 and st[57] == -6 and st[58] == -6 and (st == -4).any()
    with np.errstate(invalid="ignore"):
        assert int((fb[0, :, 3] < 0.25).sum()) >= 25


@pytest.mark.parametrize("kind,mode", KINDS)
def test_forward_bytes_are_match_ncc_full_any_alone(api, kind, mode):
    """No state leaks from the backward pass: the forward call alone on a fresh context, the new entry first on another fresh context
    (it builds whatever the pair needs lazily), and the forward call after it."""
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=16, radius=7)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        before = ctx.match_ncc_full_any(xy, FB_OFFSET, 16, 7, 3, shift=shift, mode=mode)
        path = ctx.last_path()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand, _ = ctx.match_ncc_full_fb(xy, FB_OFFSET, 16, 7, 3, shift=shift, mode=mode)
        assert ctx.last_path() == path
        after = ctx.match_ncc_full_any(xy, FB_OFFSET, 16, 7, 3, shift=shift, mode=mode)
        rec0 = ctx.match_ncc_full_any(xy, FB_OFFSET, 16, 7, 0, shift=shift, mode=mode)[0]
        swapped = ctx.match_ncc_full_any(xy, -FB_OFFSET, 16, 7, 0, shift=-shift, swap=True, mode=mode)[0]
    for got, what in ((out, "the new entry"), (after[0], "the call after it"), (rec0, "the record alone after it")):
        assert_bits_equal(got, before[0], f"{kind} mode {mode}: record of {what}")
    assert_bits_equal(cand, before[1], f"{kind} mode {mode}: candidates of the new entry")
    assert_bits_equal(after[1], before[1], f"{kind} mode {mode}: candidates of the call after it")
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        assert_bits_equal(swapped, ctx.match_ncc_full_any(xy, -FB_OFFSET, 16, 7, 0, shift=-shift, swap=True, mode=mode)[0],
                          f"{kind} mode {mode}: a swapped call after it")


def test_dev_entry_on_a_stream(api):
    import hipmem
    from hipmem import DevArray
    i0, i1, _ = class_pair("dn16")
    xy, shift = fb_points(ocw=16, radius=7)
    calls = ((7, 1), (60, 3), (7, 1), (60, 0))                     # (N, npeaks): the scratch grows, is reused, and serves fewer rows
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        want = {k: ctx.match_ncc_full_fb(xy[:k[0]], FB_OFFSET, 16, 7, k[1], shift=shift[:k[0]]) for k in set(calls)}
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        d_xy, d_sh = DevArray(src=xy), DevArray(src=shift)
        got = []
        for n, npeaks in calls:                                    # (a fresh pair: the first call builds the planes itself)
            d_out, d_fb = DevArray((n, 8), np.float32), DevArray((1 + npeaks, n, 4), np.float32)
            d_cand = DevArray((npeaks, n, 3), np.float32) if npeaks else None
            ctx.match_ncc_full_fb_dev(d_xy.ptr, n, FB_OFFSET, 16, 7, npeaks, d_out.ptr, d_fb.ptr, d_cand=d_cand.ptr if npeaks else 0,
                                      d_shift=d_sh.ptr, stream=st.value)
            got.append((d_out, d_cand, d_fb))
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == "f32i_full"
        for (n, npeaks), (d_out, d_cand, d_fb) in zip(calls, got):
            w_out, w_cand, w_fb = want[(n, npeaks)]
            assert_bits_equal(d_out.numpy(), w_out, f"_dev N {n} npeaks {npeaks}: record")
            assert_bits_equal(d_fb.numpy(), w_fb, f"_dev N {n} npeaks {npeaks}: fb")
            if npeaks:
                assert_bits_equal(d_cand.numpy(), w_cand, f"_dev N {n} npeaks {npeaks}: candidates")
        assert hipmem._hip.hipStreamDestroy(st) == 0


def test_refusals(api):
    i0, i1, path = class_pair("u8")
    xy, shift = fb_points()
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, fb, cand = np.empty((n, 8), np.float32), np.empty((9, n, 4), np.float32), np.empty((8, n, 3), np.float32)
        off = np.ascontiguousarray(FB_OFFSET)
        call = api._lib.mimc3_match_ncc_full_fb
        assert call(ctx._h, xy, n, off, None, 7, 4, 0, 0, out, None, None) == -1                          # fb NULL
        assert call(ctx._h, xy, n, off, None, 7, 4, 9, 0, out, cand.ctypes.data, fb.ctypes.data) == -1    # npeaks 9
        assert call(ctx._h, xy, n, off, None, 7, 4, 2, 0, out, None, fb.ctypes.data) == -1                # cand / npeaks mismatch
        assert call(ctx._h, xy, n, off, None, 7, 4, 0, 0, out, cand.ctypes.data, fb.ctypes.data) == -1
        assert call(ctx._h, xy, n, off, None, 7, 4, 0, 2, out, None, fb.ctypes.data) == -1                # mode 2
        assert call(ctx._h, xy, n, off, None, 8, 4, 0, 0, out, None, fb.ctypes.data) == -1                # ocw
        assert call(ctx._h, xy, n, off, None, 7, 16, 0, 0, out, None, fb.ctypes.data) == -1               # R
        bad = xy.copy()
        bad[3, 2] = 3.0                                            # the FORWARD chip leaves the image: refused, as by match_ncc_full_any
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_fb(bad, FB_OFFSET, 7, 4, 0)
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_fb(xy, (300, 0), 7, 4, 0)
        assert e.value.code == -2
        a = ctx.match_ncc_full_fb(xy, FB_OFFSET, 7, 4, 1, shift=shift)
        b = ctx.match_ncc_full_fb(xy, FB_OFFSET, 7, 4, 1, shift=shift)
        assert ctx.last_path() == path
        for x, y, what in zip(a, b, ("record", "candidates", "fb")):
            assert_bits_equal(x, y, "two identical calls after the refusals: " + what)
