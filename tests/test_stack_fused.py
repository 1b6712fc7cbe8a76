"""GPU: stack layers at any chip size and radius, accumulated in the matrix-core search's own tail (mimc3_stack_add_fused,
mimc3_stack_add_fused_dev; stack_acc.h).

By definition a fused layer is match_ncc_wide_planes(mode 0, surface) + stack_add_surfaces(surface, refused_of(record)): every comparison
below is byte for byte on everything stack_finish(k, min_count, surface=True) returns, for (k, min_count) in (4, 1), (0, 2), (8, 3) -- the
min_count steps expose cnt, count exposes lay.  Fixtures: tests/stack_fused_common.py (placed nulls: clean, box-only, chip-only, both,
refused), qualified without a device in tests/test_stack_fused_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import stack_fused_common as sf
from conftest import assert_bits_equal
from full_any_common import full_any
from full_fb_common import FB_OFFSET, class_pair, fb_points
from stack_common import misplaced, refused_of
from stack_scaled_common import NumpyScaledStack

pytestmark = pytest.mark.gpu

EINVAL, EBOUNDS, ESTATE = -1, -2, -5


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def set_pair(api, ctx, f, kind):
    """the fixture's pair on the context; "ddx": the 8-bit pair, d/dx-filtered on the device (a scaled-integer pair)"""
    ctx.set_images(f["i0"], f["i1"])
    if kind == "ddx":
        ctx.filter_images(api.CLI_KERNELS[0])


def chain_layer(ctx, xy, off, ocw, R, shift, swap=False):
    rec, _, surf = ctx.match_ncc_wide_planes(xy, off, ocw, R, 0, shift=shift, swap=swap, mode=0, surface=True)
    ctx.stack_add_surfaces(surf, refused_of(rec))
    return rec


def fused_vs_chain(api, kind, ocw, R, ocw2, nulls="placed", npts=None):
    f = sf.fixture(ocw, R, "dn12" if kind == "dn12" else "u8", nulls)
    n = f["c"].n if npts is None else npts
    xy, shift, off = np.ascontiguousarray(f["xy"][:n]), np.ascontiguousarray(f["shift"][:n]), f["off"]
    what = f"{kind} {f['what']} n {n}"
    with api.Context(0) as ctx:
        set_pair(api, ctx, f, kind)
        assert ctx.stack_fused_max_radius(ocw) == sf.max_radius(kind, ocw, api) >= R
        ctx.stack_begin_wide(n, R, shift)
        for k, (o, swap) in enumerate(sf.layers_of(f, ocw2)):
            ctx.stack_add_fused(xy, off, o, swap=swap)
            assert ctx.last_path() == sf.path_of(kind, R), what
            assert ctx.stack_info() == (n, R, k + 1)
        assert not ctx.stack_weighted()
        got = sf.finishes(ctx)
        ctx.stack_begin_wide(n, R, shift)
        recs = [chain_layer(ctx, xy, off, o, R, shift, swap) for o, swap in sf.layers_of(f, ocw2)]
        want = sf.finishes(ctx)
    for a, b, (k, mc) in zip(got, want, sf.FINISHES):
        sf.same_bytes(a, b, f"{what} npeaks {k} min_count {mc}: stack_add_fused vs the two-call chain")
    return got, recs, f


# ---- 1. fused vs chain ----
@pytest.mark.parametrize("ocw,R,ocw2", sf.U8_CASES)
def test_fused_layers_are_the_chain_s_u8(api, ocw, R, ocw2):
    got, recs, f = fused_vs_chain(api, "u8", ocw, R, ocw2)
    assert (got[0][0][:, 2] >= -1).sum() >= 20                           # (the comparison is not one of NaNs alone)
    assert recs[0][sf.REFUSED, 2] == -3 and got[0][2][sf.REFUSED] < 3 and (np.delete(got[0][2], sf.REFUSED) == 3).all()


@pytest.mark.parametrize("kind", ("dn12", "ddx"))
@pytest.mark.parametrize("ocw,R,ocw2", sf.U16_CASES)
def test_fused_layers_are_the_chain_s_u16(api, kind, ocw, R, ocw2):
    got, recs, f = fused_vs_chain(api, kind, ocw, R, ocw2)
    assert np.isfinite(got[0][3]).sum() >= 20 * (2 * R + 1) ** 2         # (the comparison is not one of NaNs alone)
    if kind == "dn12":
        assert (got[0][0][:, 2] >= -1).sum() >= 20
        assert recs[0][sf.REFUSED, 2] == -3 and got[0][2][sf.REFUSED] < 3 and (np.delete(got[0][2], sf.REFUSED) == 3).all()


# ---- 2. against NumpyStack over the CPU oracle's surfaces ----
@pytest.mark.parametrize("kind,ocw,R,ocw2", sf.ORACLE_CASES)
def test_fused_stack_is_the_definition_s(api, kind, ocw, R, ocw2):
    f = sf.fixture(ocw, R, kind)
    ref = sf.oracle_stack(f, ocw2)
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin_wide(f["c"].n, R, f["shift"])
        for o, swap in sf.layers_of(f, ocw2):
            ctx.stack_add_fused(f["xy"], f["off"], o, swap=swap)
        got = sf.finishes(ctx)
    for (rec, cand, count, mean), (k, mc) in zip(got, sf.FINISHES):
        w_rec, w_cand, w_lay, w_mean = ref.finish(k, mc)
        tag = f"{f['what']} npeaks {k} min_count {mc} vs NumpyStack over the oracle's surfaces"
        assert count.dtype == np.uint16 and np.array_equal(count, w_lay), tag + ": count"
        assert_bits_equal(mean, w_mean, tag + ": mean surface")
        assert_bits_equal(rec, w_rec, tag + ": record")
        if k:
            assert_bits_equal(cand, w_cand, tag + ": candidates")


# ---- 3. at the six chip sizes: stack_add_fused == stack_add == stack_add_class ----
SIX_LAYERS = {4: ((7, False), (7, True), (16, False)), 15: ((16, False), (16, True), (15, False)), 20: ((16, False), (16, True), (7, False))}


@pytest.mark.parametrize("radius", sorted(SIX_LAYERS))
@pytest.mark.parametrize("kind", ("u8", "dn12"))
def test_at_the_six_it_is_stack_add_and_stack_add_class(api, kind, radius):
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=16, radius=radius)
    n = xy.shape[0]
    adds = ("stack_add_fused", "stack_add") + (("stack_add_class",) if radius <= 15 else ())
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        got = {}
        for add in adds:
            ctx.stack_begin_wide(n, radius, shift)
            for ocw, swap in SIX_LAYERS[radius]:
                getattr(ctx, add)(xy, FB_OFFSET, ocw, swap=swap)
                if add == "stack_add_fused":
                    assert ctx.last_path() == sf.path_of(kind, radius)
            got[add] = sf.finishes(ctx)
    for add in adds[1:]:
        for a, b in zip(got["stack_add_fused"], got[add]):
            sf.same_bytes(a, b, f"{kind} R {radius}: stack_add_fused vs {add}")
    assert (got["stack_add_fused"][0][0][:, 2] >= -1).sum() >= 20


# ---- 4. any other pair: not fused, the kernel of match_ncc_wide_planes(mode 0) through the layer scratch ----
@pytest.mark.parametrize("kind,ocw,radius,path", (("dn16", 16, 15, "f32i_full"), ("dn16", 10, 8, "f32g_chip"), ("float", 16, 20, "f32g_wide")))
def test_fallback_runs_the_chain_s_kernel(api, kind, ocw, radius, path):
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin_wide(n, radius, shift)
        for swap in (False, True):
            ctx.stack_add_fused(xy, FB_OFFSET, ocw, swap=swap)
            assert ctx.last_path() == path
        got = sf.finishes(ctx)
        ctx.stack_begin_wide(n, radius, shift)
        for swap in (False, True):
            chain_layer(ctx, xy, FB_OFFSET, ocw, radius, shift, swap)
            assert ctx.last_path() == path
        want = sf.finishes(ctx)
    for a, b in zip(got, want):
        sf.same_bytes(a, b, f"{kind} ocw {ocw} R {radius}: the fallback vs the chain")
    assert (got[0][0][:, 2] >= -1).sum() >= 20


def test_fallback_refuses_what_no_kernel_takes(api):
    i0, i1, _ = class_pair("dn16")
    xy, shift = fb_points(ocw=16, radius=20)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin_wide(n, 20, shift)
        ctx.stack_add_fused(xy, FB_OFFSET, 16)                           # (at the six: the float wide kernel)
        assert ctx.last_path() == "f32g_wide" and ctx.stack_fused_max_radius(16) == api.wide_max_radius(16) >= 20
        before = sf.finishes(ctx)
        assert ctx.stack_fused_max_radius(10) == 15
        with pytest.raises(api.Mimc3Error) as e:
            ctx.stack_add_fused(xy, FB_OFFSET, 10)
        assert e.value.code == EINVAL and "mimc3_stack_fused_max_radius(ctx, ocw) = 15" in str(e.value)
        assert ctx.stack_info() == (n, 20, 1)
        for a, b in zip(sf.finishes(ctx), before):
            sf.same_bytes(a, b, "a refused add leaves the stack as it was")


# ---- 5. mixed and weighted ----
@pytest.mark.parametrize("kind", ("u8", "dn12"))
def test_mixed_adds_give_the_same_bytes(api, kind):
    radius, ocw = 4, 7
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, radius, shift)
        for swap in (False, True, False):
            ctx.stack_add(xy, FB_OFFSET, ocw, swap=swap)
        want = sf.finishes(ctx)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add(xy, FB_OFFSET, ocw)
        ctx.stack_add_fused(xy, FB_OFFSET, ocw, swap=True)
        assert ctx.last_path() == sf.path_of(kind, radius)
        chain_layer(ctx, xy, FB_OFFSET, ocw, radius, shift)
        for a, b in zip(sf.finishes(ctx), want):
            sf.same_bytes(a, b, f"{kind}: stack_add, stack_add_fused, stack_add_surfaces vs three stack_add")


@pytest.mark.parametrize("kind", ("u8", "dn12"))
def test_fused_layer_on_a_weighted_stack(api, kind):
    """One stack_add_surfaces_scaled at weight 3 (scale 1, the stack's radius), then a fused layer: NumpyScaledStack's bytes"""
    radius, ocw = 4, 7
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    o_rec, _, o_surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 0, shift=shift, swap=True)
    c_rec, _, c_surf, _ = full_any(i0, i1, xy, FB_OFFSET, ocw, radius, 0, shift=shift)
    ref = NumpyScaledStack(n, radius, shift).add_scaled(o_surf, radius, 1.0, 3.0, refused_of(o_rec)).add(c_surf, refused_of(c_rec))
    assert ref.weighted
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add_surfaces_scaled(o_surf, radius, 1.0, 3.0, refused_of(o_rec))
        assert ctx.stack_weighted()
        ctx.stack_add_fused(xy, FB_OFFSET, ocw)
        assert ctx.stack_weighted() and ctx.last_path() == sf.path_of(kind, radius) and ctx.stack_info() == (n, radius, 2)
        got = sf.finishes(ctx)
    for (rec, cand, count, mean), (k, mc) in zip(got, sf.FINISHES):
        w_rec, w_cand, w_lay, w_mean = ref.finish(k, mc)
        tag = f"{kind}: weighted, npeaks {k} min_count {mc} vs NumpyScaledStack"
        assert np.array_equal(count, w_lay), tag
        assert_bits_equal(mean, w_mean, tag + ": mean surface")
        assert_bits_equal(rec, w_rec, tag + ": record")
        if k:
            assert_bits_equal(cand, w_cand, tag + ": candidates")


# ---- 6. launch-shape edges ----
@pytest.mark.parametrize("kind,ocw,R,ocw2", (("u8", 10, 4, 7), ("u8", 7, 16, 9), ("dn12", 10, 15, 12), ("dn12", 16, 20, 15)))
@pytest.mark.parametrize("npts", (1, 13))
def test_grids_that_are_no_multiple_of_eight(api, kind, ocw, R, ocw2, npts):
    fused_vs_chain(api, kind, ocw, R, ocw2, npts=npts)


@pytest.mark.parametrize("kind,ocw,R,ocw2", (("u8", 10, 4, 7), ("u8", 7, 16, 9), ("dn12", 10, 15, 12), ("dn12", 16, 20, 15)))
def test_every_point_dirty_and_every_point_refused(api, kind, ocw, R, ocw2):
    got, recs, f = fused_vs_chain(api, kind, ocw, R, ocw2, nulls="all")
    assert (got[0][2] == 3).all() and (got[0][0][:, 2] >= -1).sum() >= 20
    f = sf.fixture(ocw, R, "dn12" if kind == "dn12" else "u8", "refused")
    n = f["c"].n
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin_wide(n, R, f["shift"])
        for _ in range(2):
            ctx.stack_add_fused(f["xy"], f["off"], ocw)
        assert ctx.last_path() == sf.path_of(kind, R) and ctx.stack_info() == (n, R, 2)
        rec, _, count, mean = ctx.stack_finish(0, 1, surface=True)
    assert (count == 0).all() and (rec[:, 2] == -3).all() and np.isnan(mean).all()


# ---- 7. the _dev entry ----
@pytest.mark.parametrize("kind,ocw,R", (("u8", 10, 4), ("u8", 7, 16), ("dn12", 10, 15), ("dn12", 16, 20)))
def test_dev_entry_and_a_chip_that_leaves_the_image(api, kind, ocw, R):
    import hipmem
    from hipmem import DevArray
    f = sf.fixture(ocw, R, kind)
    n, xy, shift, off = f["c"].n, f["xy"], f["shift"], f["off"]
    out = 9                                                              # a clean point
    bad = xy.copy()
    bad[out, 2] = 2.0                                                    # its chip leaves the image: only the _dev entry takes the row
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_fused(xy, off, ocw)
        ctx.stack_add_fused(xy, off, ocw, swap=True)
        want = sf.finishes(ctx)
        with pytest.raises(api.Mimc3Error) as e:
            ctx.stack_add_fused(bad, off, ocw)
        assert e.value.code == EBOUNDS and ctx.stack_info() == (n, R, 2)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        d_xy, d_bad = DevArray(src=np.ascontiguousarray(xy)), DevArray(src=np.ascontiguousarray(bad))
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_fused_dev(d_xy.ptr, n, off, ocw, stream=st.value)
        ctx.stack_add_fused_dev(d_xy.ptr, n, off, ocw, stream=st.value, swap=True)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == sf.path_of(kind, R) and ctx.stack_info() == (n, R, 2)
        for a, b in zip(sf.finishes(ctx), want):
            sf.same_bytes(a, b, f"{f['what']}: _dev on a stream of its own vs the host entry")
        # the row whose chip leaves the image: the layer counts, its cells get nothing, every other point is the host entry's
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_fused_dev(d_bad.ptr, n, off, ocw, stream=st.value)
        ctx.stack_add_fused_dev(d_xy.ptr, n, off, ocw, stream=st.value, swap=True)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        rec1, _, count1, mean1 = ctx.stack_finish(0, 1, surface=True)
        rec2, _, count2, mean2 = ctx.stack_finish(0, 2, surface=True)
        assert hipmem._hip.hipStreamDestroy(st) == 0
    w1, w2 = want[0], want[1]                                            # (npeaks 4, min_count 1), (0, 2)
    assert np.array_equal(count1, w1[2]) and count1[out] == 2            # the layer counts ...
    assert np.isnan(mean2[out]).all() and np.isfinite(mean1[out]).any()  # ... but no cell has two values: the bad row added none
    others = np.arange(n) != out
    assert mean1[others].tobytes() == w1[3][others].tobytes() and mean2[others].tobytes() == w2[3][others].tobytes()
    assert rec2[others].tobytes() == w2[0][others].tobytes()


# ---- 8. refusals: the stack's bytes and stack_info stay as they were ----
def test_refusals_leave_the_stack_untouched(api):
    from hipmem import DevArray
    f = sf.fixture(10, 4, "u8")
    n, xy, shift, off = f["c"].n, np.ascontiguousarray(f["xy"]), f["shift"], f["off"]
    call, dev = api._lib.mimc3_stack_add_fused, api._lib.mimc3_stack_add_fused_dev
    with api.Context(0) as ctx:
        ctx.stack_begin(n, 4, shift)
        assert call(ctx._h, xy, n, off, 10, 0) == ESTATE and ctx.stack_fused_max_radius(10) == 0      # no images
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin(0, 4)
        assert call(ctx._h, xy, n, off, 10, 0) == ESTATE                 # no stack
        ctx.stack_begin(n, 4, shift)
        ctx.stack_add_fused(xy, off, 10)
        want = sf.finishes(ctx)
        d_xy = DevArray(src=xy)
        assert call(ctx._h, np.ascontiguousarray(xy[:5]), 5, off, 10, 0) == EINVAL          # N differs from the stack's
        assert dev(ctx._h, d_xy.ptr, 5, 1, -1, 10, 0, None) == EINVAL
        for ocw in (0, 81, -3):
            assert call(ctx._h, xy, n, off, ocw, 0) == EINVAL and dev(ctx._h, d_xy.ptr, n, 1, -1, ocw, 0, None) == EINVAL
            assert ctx.stack_fused_max_radius(ocw) == 0
        assert dev(ctx._h, None, n, 1, -1, 10, 0, None) == EINVAL         # null pointers
        assert dev(None, d_xy.ptr, n, 1, -1, 10, 0, None) == EINVAL
        assert call(ctx._h, xy, 0, off, 10, 0) == EINVAL
        bad = xy.copy()
        bad[3, 2] = 3.0
        assert call(ctx._h, bad, n, off, 10, 0) == EBOUNDS               # a chip that leaves the image
        assert call(ctx._h, xy, n, np.array([700, 0], np.int32), 10, 0) == EBOUNDS          # a box that leaves the zero border
        assert ctx.stack_info() == (n, 4, 1)
        for a, b in zip(sf.finishes(ctx), want):
            sf.same_bytes(a, b, "a refused add leaves the stack as it was")


def test_a_full_stack_refuses_the_layer(api):
    """65,535 layers of one point's 3 x 3 surface, then the fused add: MIMC3_ESTATE, the stack as it was"""
    from hipmem import DevArray
    f = sf.fixture(10, 4, "u8")
    xy, off = np.ascontiguousarray(f["xy"][7:8]), f["off"]
    d_surf = DevArray(src=np.full((1, 9), 0.5, np.float32))
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin(1, 1)
        add = api._lib.mimc3_stack_add_surfaces_dev
        for _ in range(65535):
            assert add(ctx._h, d_surf.ptr, None, 1, None) == 0
        assert ctx.stack_info() == (1, 1, 65535)
        before = ctx.stack_finish(0, 1, surface=True)
        assert api._lib.mimc3_stack_add_fused(ctx._h, xy, 1, off, 10, 0) == ESTATE
        assert ctx.stack_info() == (1, 1, 65535)
        sf.same_bytes(ctx.stack_finish(0, 1, surface=True), before, "a full stack")


# ---- 9. what it buys: the five (34, -27) px pairs at R 40, ocw 7 ----
def test_far_series_through_the_fused_entry(api):
    from test_wide_stack_cpu import FAR_STACK_OCW, FAR_STACK_R, far_series
    from stack_common import NumpyStack
    from wide_common import FAR_TRUE
    series = far_series()
    n = series[0].n
    ref = NumpyStack(n, FAR_STACK_R)
    for c in series:
        rec, _, surf, _ = full_any(c.i0, c.i1, c.xyuvav, (0, 0), FAR_STACK_OCW, FAR_STACK_R, 0)
        ref.add(surf, refused_of(rec))
    want = int(misplaced(ref.finish(0, 1)[0], FAR_TRUE).sum())
    with api.Context(0) as ctx:
        ctx.stack_begin_wide(n, FAR_STACK_R)
        for c in series:
            ctx.set_images(c.i0, c.i1)
            ctx.stack_add_fused(c.xyuvav, (0, 0), FAR_STACK_OCW)
            assert ctx.last_path() == "u8_mfma_wide"
        rec = ctx.stack_finish(0, 1)[0]
    got = int(misplaced(rec, FAR_TRUE).sum())
    print(f"R {FAR_STACK_R}, ocw {FAR_STACK_OCW}: misplaced after stacking {got} of {n} points (the CPU definition: {want})")
    assert got == want
