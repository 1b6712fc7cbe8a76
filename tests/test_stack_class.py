"""GPU: stack layers through the kernel of the pair's class (mimc3_stack_add_class, mimc3_stack_add_class_dev).

The accumulation adds only finite cells and takes the refused points from the record, and the class kernels' finite cells and records
are the float kernel's bit for bit: the stack after stack_add_class is, byte for byte in everything stack_finish returns, the stack after
stack_add -- on every pixel class, mixed with the other adds, on a weighted stack, and beyond R 15, where the call is stack_add.  On
the integer classes both equal the numpy definition (tests/stack_common.py) over the float oracle's surfaces."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import full_any
from full_fb_common import FB_OFFSET, class_pair, fb_points
from stack_common import NumpyStack, refused_of
from stack_scaled_common import NumpyScaledStack

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
WHAT = ("record", "candidates", "count", "mean surface")
# stack R -> the grid's chip size and the three layers (ocw, swap): raw, swapped back, another chip size
LAYERS = {4: (16, ((7, False), (7, True), (16, False))), 15: (16, ((16, False), (16, True), (15, False)))}


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def same_bytes(a, b, what):
    for x, y, name in zip(a, b, WHAT):
        assert (x is None) == (y is None), f"{what}: {name}"
        if x is not None:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {name}"


def finishes(ctx):
    return [ctx.stack_finish(k, mc, surface=True) for k, mc in ((4, 1), (0, 2), (8, 3))]


@pytest.mark.parametrize("radius", sorted(LAYERS))
@pytest.mark.parametrize("kind", ("u8", "dn12", "dn16", "float"))
def test_class_layers_are_stack_add_s(api, kind, radius):
    i0, i1, path = class_pair(kind)
    grid_ocw, layers = LAYERS[radius]
    xy, shift = fb_points(ocw=grid_ocw, radius=radius)
    n = xy.shape[0]
    what = f"{kind} R {radius}"
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        got = {}
        for cls in (False, True):
            ctx.stack_begin(n, radius, shift)
            for ocw, swap in layers:
                (ctx.stack_add_class if cls else ctx.stack_add)(xy, FB_OFFSET, ocw, swap=swap)
                assert ctx.last_path() == (path if cls else "f32g_full"), what
            assert ctx.stack_info() == (n, radius, len(layers)) and not ctx.stack_weighted()
            got[cls] = finishes(ctx)
        for a, b in zip(got[True], got[False]):
            same_bytes(a, b, what + ": stack_add_class vs stack_add")
        rec = got[True][0][0]
        assert (rec[:, 2] >= -1).sum() >= 20                             # (the comparison is not one of NaNs alone)
        if kind == "float":
            return                                                       # (the oracle's float surface is the device's within 1 ulp only)
        ref = NumpyStack(n, radius, shift)
        for ocw, swap in layers:
            o_rec, _, o_surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 0, shift=shift, swap=swap)
            ref.add(o_surf, refused_of(o_rec))
        for (rec, cand, count, mean), (k, mc) in zip(got[True], ((4, 1), (0, 2), (8, 3))):
            w_rec, w_cand, w_lay, w_mean = ref.finish(k, mc)
            tag = f"{what} npeaks {k} min_count {mc} vs NumpyStack over the oracle's surfaces"
            assert count.dtype == np.uint16 and np.array_equal(count, w_lay), tag + ": count"
            assert_bits_equal(mean, w_mean, tag + ": mean surface")
            assert_bits_equal(rec, w_rec, tag + ": record")
            if k:
                assert_bits_equal(cand, w_cand, tag + ": candidates")


@pytest.mark.parametrize("kind", ("u8", "dn12", "dn16"))
def test_mixed_adds_give_the_same_bytes(api, kind):
    """stack_add, stack_add_class and stack_add_surfaces (of match_ncc_full_surf's surface) in one stack == three stack_add"""
    radius, ocw = 4, 7
    i0, i1, path = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, radius, shift)
        for swap in (False, True, False):
            ctx.stack_add(xy, FB_OFFSET, ocw, swap=swap)
        want = finishes(ctx)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add(xy, FB_OFFSET, ocw)
        ctx.stack_add_class(xy, FB_OFFSET, ocw, swap=True)
        rec, _, surf = ctx.match_ncc_full_surf(xy, FB_OFFSET, ocw, radius, 0, shift=shift)
        assert ctx.last_path() == path
        ctx.stack_add_surfaces(surf, refused_of(rec))
        for a, b in zip(finishes(ctx), want):
            same_bytes(a, b, f"{kind}: mixed adds")


@pytest.mark.parametrize("kind", ("u8", "dn16"))
def test_class_layer_on_a_weighted_stack(api, kind):
    """One stack_add_surfaces_scaled at weight 3 (scale 1, the stack's radius), then a class layer: NumpyScaledStack, and stack_add's bytes"""
    radius, ocw = 4, 7
    i0, i1, path = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    o_rec, _, o_surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 0, shift=shift, swap=True)
    c_rec, _, c_surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 0, shift=shift)
    ref = NumpyScaledStack(n, radius, shift).add_scaled(o_surf, radius, 1.0, 3.0, refused_of(o_rec)).add(c_surf, refused_of(c_rec))
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        got = {}
        for cls in (False, True):
            ctx.stack_begin(n, radius, shift)
            ctx.stack_add_surfaces_scaled(o_surf, radius, 1.0, 3.0, refused_of(o_rec))
            assert ctx.stack_weighted()
            (ctx.stack_add_class if cls else ctx.stack_add)(xy, FB_OFFSET, ocw)
            assert ctx.stack_weighted() and ctx.last_path() == (path if cls else "f32g_full")
            got[cls] = finishes(ctx)
        for a, b in zip(got[True], got[False]):
            same_bytes(a, b, f"{kind}: weighted, stack_add_class vs stack_add")
        assert ref.weighted
        rec, cand, count, mean = got[True][0]
        w_rec, w_cand, w_lay, w_mean = ref.finish(4, 1)
        assert np.array_equal(count, w_lay)
        assert_bits_equal(mean, w_mean, f"{kind}: weighted mean vs NumpyScaledStack")
        assert_bits_equal(rec, w_rec, f"{kind}: weighted record vs NumpyScaledStack")
        assert_bits_equal(cand, w_cand, f"{kind}: weighted candidates vs NumpyScaledStack")


def test_beyond_radius_15_it_is_stack_add(api):
    radius, ocw = 16, 7
    i0, i1, _ = class_pair("u8")
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        got = {}
        for cls in (False, True):
            ctx.stack_begin_wide(n, radius, shift)
            for swap in (False, True):
                (ctx.stack_add_class if cls else ctx.stack_add)(xy, FB_OFFSET, ocw, swap=swap)
                assert ctx.last_path() == "f32g_wide"
            got[cls] = finishes(ctx)
        for a, b in zip(got[True], got[False]):
            same_bytes(a, b, "R 16: stack_add_class vs stack_add")
        assert (got[True][0][0][:, 2] >= -1).sum() >= 20


def test_dev_entry_and_refusals(api):
    import hipmem
    from hipmem import DevArray
    radius, ocw = 4, 7
    i0, i1, path = class_pair("dn12")
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    off = np.ascontiguousarray(FB_OFFSET, np.int32)
    call, dev = api._lib.mimc3_stack_add_class, api._lib.mimc3_stack_add_class_dev
    with api.Context(0) as ctx:
        ctx.stack_begin(n, radius, shift)
        assert call(ctx._h, np.ascontiguousarray(xy), n, off, ocw, 0) == ESTATE             # no images
        ctx.set_images(i0, i1)
        ctx.stack_begin(0, radius)
        assert call(ctx._h, np.ascontiguousarray(xy), n, off, ocw, 0) == ESTATE             # no stack
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add_class(xy, FB_OFFSET, ocw)
        want = finishes(ctx)
        assert call(ctx._h, np.ascontiguousarray(xy[:5]), 5, off, ocw, 0) == EINVAL         # N differs from the stack's
        assert call(ctx._h, np.ascontiguousarray(xy), n, off, 8, 0) == EINVAL               # ocw 8
        assert dev(ctx._h, None, n, 0, 0, ocw, 0, None) == EINVAL
        for a, b in zip(finishes(ctx), want):
            same_bytes(a, b, "a refused add leaves the stack as it was")
        d_xy = DevArray(src=np.ascontiguousarray(xy))
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add_class_dev(d_xy.ptr, n, FB_OFFSET, ocw, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == path and ctx.stack_info() == (n, radius, 1)
        for a, b in zip(finishes(ctx), want):
            same_bytes(a, b, "_dev on a stream of its own vs the host entry")
        assert hipmem._hip.hipStreamDestroy(st) == 0
