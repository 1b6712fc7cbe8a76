"""GPU: the scaled and weighted layers of NCC stacking (mimc3_stack_add_scaled, mimc3_stack_add_surfaces_scaled; stack_add_scaled_kernel
in stack_kernel.hip).

Every comparison is bit for bit (NaNs by position).  Scale 1, weight 1 at the stack's radius is stack_add; any other layer is what the
numpy definition (tests/stack_scaled_common.py) makes of the device's own layer surfaces, which match_ncc_wide(..., surface=True) serves
around stack_layer_shift; the host entry is that search chained with stack_add_surfaces_scaled; crafted surfaces exercise NaN, Inf,
zero-weight taps and long fractions; the lazy plane of the weights' sums; the chunk edge at stack_chunk(46) + 61 points; refusals leave
the stack's bytes and its weighted flag alone; the _dev entries on a stream of their own; the series over six time baselines."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_fb_common import FB_OFFSET, class_pair, fb_pair, fb_points
from stack_common import misplaced, refused_of
from stack_scaled_common import (SCALED_COUNTS, SCALED_MOTION, SCALED_OCW, SCALED_R, NumpyScaledStack, layer_radius, layer_shift, layer_truth,
                                 resample, scaled_series_pairs, scaled_series_points)

pytestmark = pytest.mark.gpu

EINVAL, EBOUNDS, ESTATE = -1, -2, -5
WHAT = ("record", "candidates", "count", "surface")


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def begin(ctx, n, radius, shift):
    (ctx.stack_begin_wide if radius > 15 else ctx.stack_begin)(n, radius, shift)


def same_bytes(a, b, what):
    for x, y, name in zip(a, b, WHAT):
        if x is None:
            assert y is None, f"{what}: {name}"
        else:
            assert x.tobytes() == y.tobytes(), f"{what}: {name}"


def check_finish(ctx, ref, what, npeaks_list=(0, 3), min_counts=(1,)):
    """ctx's stack against the numpy stack `ref`: the weighted flag, record, candidates, count and mean surface"""
    assert ctx.stack_info() == (ref.n, ref.radius, ref.layers), what
    assert ctx.stack_weighted() == ref.weighted, what
    for mc in min_counts:
        for npeaks in npeaks_list:
            rec, cand, count, surf = ctx.stack_finish(npeaks, mc, surface=True)
            w_rec, w_cand, w_lay, w_mean = ref.finish(npeaks, mc)
            tag = f"{what}: npeaks {npeaks} min_count {mc}"
            assert np.array_equal(count, w_lay), tag + ": count"
            assert_bits_equal(surf, w_mean, tag + ": mean surface")
            assert_bits_equal(rec, w_rec, tag + ": record")
            assert (cand is None) == (npeaks == 0)
            if npeaks:
                assert_bits_equal(cand, w_cand, tag + ": candidates")
    return rec, surf


# ---- 1. scale 1, weight 1 at the stack's radius is stack_add ----
@pytest.mark.parametrize("ocw,radius", ((7, 4), (16, 15), (7, 16)))
@pytest.mark.parametrize("kind", ("u8", "float"))
def test_scale_one_is_stack_add(api, kind, ocw, radius):
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for pts, sh_all in ((xy, shift), (xy[:1], shift[:1])):           # 60 points, and N = 1
            for sh in (sh_all, None):
                got = []
                for scaled in (False, True):
                    begin(ctx, pts.shape[0], radius, sh)
                    if scaled:
                        assert api.stack_layer_radius(radius, 1.0) == radius
                        ctx.stack_add_scaled(pts, FB_OFFSET, ocw, 1.0, 1.0, radius=radius)
                        ctx.stack_add_scaled(pts, FB_OFFSET, ocw, 1.0, swap=True)
                    else:
                        ctx.stack_add(pts, FB_OFFSET, ocw)
                        ctx.stack_add(pts, FB_OFFSET, ocw, swap=True)
                    assert ctx.last_path() == ("f32g_wide" if radius > 15 else "f32g_full")
                    assert ctx.stack_info() == (pts.shape[0], radius, 2) and not ctx.stack_weighted()
                    got.append([ctx.stack_finish(k, mc, surface=True) for k in (0, 8) for mc in (1, 2)])
                for a, b in zip(*got):
                    same_bytes(b, a, f"{kind} ocw {ocw} R {radius} N {pts.shape[0]} shift {sh is not None}")
                if pts.shape[0] > 1:
                    assert (got[0][0][0][:, 2] >= -1).sum() >= 20         # (the comparison is not one of NaNs alone)


# ---- 2. the definition, on the device's own layer surfaces ----
# (pair, ocw, stack R, layers (scale, layer radius or None = stack_layer_radius, weight)): every fixture holds a layer two below its
# stack_layer_radius, so outer cells get no count from it
DEFINITION = {
    "R4-half-2-1.5": ("u8", 7, 4, ((0.5, None, 1.0), (2.0, None, 1.0), (1.5, 5, 1.0))),
    "R4-third-2.5-2": ("float", 7, 4, ((1 / 3, None, 1.0), (2.5, None, 1.0), (2.0, 7, 1.0))),
    "R6-wide-layer": ("float", 7, 6, ((2.5, None, 1.0), (2.5, 14, 1.0), (1.0, None, 1.0))),          # Rl 16: the wide kernel's layer
    "R16-narrow-layer": ("u8", 7, 16, ((0.5, None, 1.0), (0.5, 7, 1.0), (1.0, None, 1.0))),          # Rl 9 into the wide tail
    "ocw40": ("u8", 40, 4, ((2.0, None, 1.0), (0.5, None, 1.0), (1.5, 5, 1.0))),
    "R4-weights": ("u8", 7, 4, ((0.5, None, 0.25), (2.0, None, 1.0), (1.5, 5, 3.5))),
}


@pytest.mark.parametrize("name", DEFINITION)
def test_against_the_numpy_definition(api, name):
    kind, ocw, radius, layers = DEFINITION[name]
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    ref = NumpyScaledStack(n, radius, shift)
    taps_seen, left_out, paths = set(), 0, set()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        begin(ctx, n, radius, shift)
        for s, Rl, w in layers:
            full = api.stack_layer_radius(radius, s)
            assert full == layer_radius(radius, s)
            Rl = full if Rl is None else Rl
            lsh = ctx.stack_layer_shift(s)
            assert lsh.dtype == np.int32 and np.array_equal(lsh, layer_shift(shift, s)), s
            rec, _, surf = ctx.match_ncc_wide(xy, FB_OFFSET, ocw, Rl, 0, shift=lsh, surface=True)
            ref.add_scaled(surf, Rl, s, w, refused_of(rec))
            _, read, taps = resample(surf, Rl, shift, radius, s)
            taps_seen |= set(np.unique(taps[read]).tolist())
            left_out += int((~read).sum())
            ctx.stack_add_scaled(xy, FB_OFFSET, ocw, s, w, radius=Rl)
            paths.add(ctx.last_path())
        # the fixture holds what it is for: cells of one, two and four taps, cells a layer leaves out, different counts, finite means
        assert taps_seen == {1, 2, 4} and left_out > 0, (taps_seen, left_out)
        assert (ref.cnt == 3).any() and ((ref.cnt > 0) & (ref.cnt < 3)).any()
        if name == "R6-wide-layer":
            assert paths == {"f32g_wide", "f32g_full"}
        rec, mean = check_finish(ctx, ref, name, min_counts=(1, 3))
    assert np.isfinite(ref.mean(1)).mean() > 0.5 and np.isnan(mean).any() and np.isfinite(mean).any()
    assert (ref.finish(0, 1)[0][:, 2] >= -1).sum() >= 10


# ---- 3. the host entry is the search chained with stack_add_surfaces_scaled ----
def test_add_scaled_is_search_then_add_surfaces_scaled(api):
    ocw, radius = 7, 4
    i0, i1 = fb_pair()
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    u, v = int(xy[40, 2]), int(xy[40, 3])
    i0[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1] = 0                      # the chip of point 40 is null: refused by the forward searches
    layers = ((1.5, 2.5, False), (2.0, 1.0, True), (0.5, 2.5, False))
    got = []
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for chained in (False, True):
            ctx.stack_begin(n, radius, shift)
            for s, w, swap in layers:
                Rl = api.stack_layer_radius(radius, s)
                if chained:
                    rec, _, surf = ctx.match_ncc_wide(xy, FB_OFFSET, ocw, Rl, 0, shift=ctx.stack_layer_shift(s), swap=swap, surface=True)
                    assert swap or rec[40, 2] == -3
                    ctx.stack_add_surfaces_scaled(surf, Rl, s, w, refused=refused_of(rec))
                else:
                    ctx.stack_add_scaled(xy, FB_OFFSET, ocw, s, w, swap=swap)
            assert ctx.stack_info() == (n, radius, 3) and ctx.stack_weighted()
            got.append([ctx.stack_finish(k, mc, surface=True) for k in (0, 3) for mc in (1, 3)])
    for a, b in zip(*got):
        same_bytes(b, a, "chained")
    rec, _, count, _ = got[0][0]
    assert count[40] < 3 and (count == 3).sum() >= 40 and (rec[:, 2] >= -1).sum() >= 20


# ---- 4. crafted surfaces ----
@pytest.mark.parametrize("radius", (1, 2))
def test_crafted_surfaces(api, radius):
    """Eight points whose shifts (0, 7, -13, 1, ...) give pu long fractions and negative values at scale 0.1; layers with NaN and +-Inf
    taps; a scale-2 layer at radius 2 R, one below stack_layer_radius: every pu is an integer, the second tap has weight zero and lies
    on a NaN row or outside the layer, and every cell counts; a refused point."""
    n, S = 8, 2 * radius + 1
    shift = np.array([[0, 0], [7, -13], [-13, 7], [1, -1], [5, 5], [-6, 3], [2, 0], [0, 9]], np.int32)
    rng = np.random.default_rng(radius)
    refused = np.zeros(n, bool)
    refused[6] = True
    ref = NumpyScaledStack(n, radius, shift)
    layers = []
    for s in (0.1, 0.1, 0.7, 1.0):
        Rl = layer_radius(radius, s)
        L = (rng.random((n, (2 * Rl + 1) ** 2)) - 0.3).astype(np.float32)
        layers.append((L, Rl, s, 1.0))
    layers[0][0][0, 4], layers[0][0][1, 0], layers[0][0][2, 8] = np.nan, np.inf, -np.inf
    layers[1][0][3, :3], layers[1][0][4, 4] = (np.inf, -np.inf, np.nan), np.inf
    Rl = 2 * radius                                                       # scale 2: taps at ju = 2 su + 2 R alone
    holes = (rng.random((n, 2 * Rl + 1, 2 * Rl + 1)) - 0.3).astype(np.float32)
    holes[:, 1::2, :] = np.nan
    holes[:, :, 1::2] = np.nan
    assert layer_radius(radius, 2.0) == Rl + 1
    layers.append((holes.reshape(n, -1), Rl, 2.0, 1.0))
    with api.Context(0) as ctx:                                           # (no images: add_surfaces_scaled needs none)
        ctx.stack_begin(n, radius, shift)
        for L, Rl, s, w in layers:
            before = ref.cnt.copy()
            ref.add_scaled(L, Rl, s, w, refused)
            ctx.stack_add_surfaces_scaled(L, Rl, s, w, refused=refused)
        assert ((ref.cnt - before) == 1).all()                            # the scale-2 layer: every cell, whatever lies beside its tap
        rec, mean = check_finish(ctx, ref, f"R {radius}", min_counts=(1, 2, 5))
    assert ref.lay.tolist() == [5, 5, 5, 5, 5, 5, 0, 5] and rec[6, 2] == -3
    assert (ref.cnt < 5).any() and (ref.cnt == 5).any() and np.isnan(mean).any() and np.isfinite(mean).any()
    # long fractions and negative pu at scale 0.1: 0.1 * (7 - 1) - 1 and 0.1 * (-13 + 1) + 1
    _, _, taps = resample(layers[0][0], layers[0][1], shift, radius, 0.1)
    assert (taps[1] == 4).all() and (taps[0].reshape(S, S)[radius, radius] == 1)


# ---- 5. weights: the lazy plane of the weights' sums ----
def test_weights(api):
    ocw, radius = 7, 4
    i0, i1 = fb_pair()
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n, NC = xy.shape[0], (2 * radius + 1) ** 2
    rng = np.random.default_rng(5)
    extra = (rng.random((n, NC)) - 0.3).astype(np.float32)
    extra[rng.random(extra.shape) < 0.05] = np.nan

    def layer(ctx, s):
        Rl = api.stack_layer_radius(radius, s)
        rec, _, surf = ctx.match_ncc_wide(xy, FB_OFFSET, ocw, Rl, 0, shift=ctx.stack_layer_shift(s), surface=True)
        return surf, Rl, refused_of(rec)

    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        # two unweighted layers, then weight 3.5: wsum starts from cnt; then an old add on the weighted stack
        ctx.stack_begin(n, radius, shift)
        ref = NumpyScaledStack(n, radius, shift)
        surf, _, rf = layer(ctx, 1.0)
        ctx.stack_add(xy, FB_OFFSET, ocw)
        ref.add(surf, rf)
        ctx.stack_add_surfaces(extra, np.arange(n) % 4 == 0)
        ref.add(extra, np.arange(n) % 4 == 0)
        assert not ctx.stack_weighted()
        check_finish(ctx, ref, "two unweighted layers")
        surf, Rl, rf = layer(ctx, 1.5)
        ctx.stack_add_scaled(xy, FB_OFFSET, ocw, 1.5, 3.5)
        ref.add_scaled(surf, Rl, 1.5, 3.5, rf)
        assert ctx.stack_weighted()
        check_finish(ctx, ref, "then weight 3.5", min_counts=(1, 3))
        surf, _, rf = layer(ctx, 1.0)
        ctx.stack_add(xy, FB_OFFSET, ocw, swap=False)
        ref.add(surf, rf)
        ctx.stack_add_surfaces(extra)
        ref.add(extra)
        check_finish(ctx, ref, "then stack_add and stack_add_surfaces", min_counts=(1, 5))
        ctx.stack_begin(n, radius, shift)
        assert not ctx.stack_weighted() and ctx.stack_info() == (n, radius, 0)
        # weights (0.25, 1, 3.5) against numpy
        ref = NumpyScaledStack(n, radius, shift)
        for s, w in ((0.5, 0.25), (2.0, 1.0), (1.5, 3.5)):
            surf, Rl, rf = layer(ctx, s)
            ctx.stack_add_scaled(xy, FB_OFFSET, ocw, s, w)
            ref.add_scaled(surf, Rl, s, w, rf)
        check_finish(ctx, ref, "weights 0.25, 1, 3.5", min_counts=(1, 3))
        # weight 2 on every layer: the unweighted stack's bytes
        got = []
        for w in (1.0, 2.0):
            ctx.stack_begin(n, radius, shift)
            for s in (0.5, 2.0, 1.5):
                ctx.stack_add_scaled(xy, FB_OFFSET, ocw, s, w, radius=api.stack_layer_radius(radius, s) - (2 if s == 2.0 else 0))
            assert ctx.stack_weighted() == (w == 2.0)
            got.append([ctx.stack_finish(k, mc, surface=True) for k in (0, 3) for mc in (1, 3)])
        for a, b in zip(*got):
            same_bytes(b, a, "weight 2 everywhere")
        ctx.stack_begin(0, 0)
        assert not ctx.stack_weighted()


# ---- 6. the chunk edge ----
def test_chunk_edge(api):
    """Stack R 15, scale 3, ocw 7, layer radius 46: the chunk is stack_chunk(46) = 7,281 points, N = 7,281 + 61 -- the second launch of
    the search and of the accumulation holds 61 points.  The 60 points over and over: every copy's bytes are the first copy's, and the
    first copy's are numpy's."""
    ocw, radius, s = 7, 15, 3.0
    Rl = api.stack_layer_radius(radius, s)
    assert Rl == 46 and api.stack_chunk(Rl) == 7281 < api.stack_chunk(radius)
    i0, i1 = fb_pair()
    base, bshift = fb_points(ocw=ocw, radius=radius)
    n = api.stack_chunk(Rl) + 61
    idx = np.arange(n) % 60
    xy, shift = np.ascontiguousarray(base[idx]), np.ascontiguousarray(bshift[idx])
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add_scaled(xy, FB_OFFSET, ocw, s, 1.5)
        assert ctx.last_path() == "f32g_wide" and ctx.stack_info() == (n, radius, 1) and ctx.stack_weighted()
        rec, cand, count, mean = ctx.stack_finish(2, 1, surface=True)
        w_rec, _, surf = ctx.match_ncc_wide(base, FB_OFFSET, ocw, Rl, 0, shift=layer_shift(bshift, s), surface=True)
    ref = NumpyScaledStack(60, radius, bshift).add_scaled(surf, Rl, s, 1.5, refused_of(w_rec))
    f_rec, f_cand, f_lay, f_mean = ref.finish(2, 1)
    assert np.array_equal(count[:60], f_lay)
    assert_bits_equal(mean[:60], f_mean, "first copy: mean surface")
    assert_bits_equal(rec[:60], f_rec, "first copy: record")
    assert_bits_equal(cand[:, :60], f_cand, "first copy: candidates")
    assert mean.tobytes() == mean[:60][idx].tobytes() and rec.tobytes() == rec[:60][idx].tobytes() and np.array_equal(count, count[:60][idx])
    assert np.isfinite(f_mean).mean() > 0.3 and (f_lay > 0).sum() >= 20


# ---- 7. refusals ----
def test_refusals(api):
    ocw, radius = 7, 4
    i0, i1 = fb_pair()
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n = xy.shape[0]
    surf = np.zeros((n, 81), np.float32)

    def code(fn, *a, **k):
        with pytest.raises(api.Mimc3Error) as e:
            fn(*a, **k)
        return e.value.code

    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        # no stack
        assert code(ctx.stack_add_scaled, xy, FB_OFFSET, ocw, 2.0, radius=9) == ESTATE
        assert code(ctx.stack_add_surfaces_scaled, surf, 4, 1.0) == ESTATE
        assert code(ctx.stack_layer_shift, 2.0) == ESTATE and not ctx.stack_weighted()
        for weighted in (False, True):
            ctx.stack_begin(n, radius, shift)
            ctx.stack_add_scaled(xy, FB_OFFSET, ocw, 2.0, 2.5 if weighted else 1.0)
            assert ctx.stack_weighted() == weighted
            before = ctx.stack_finish(3, 1, surface=True)
            for s in (0.0, -1.0, float("nan"), 2.0 ** 7):
                assert code(ctx.stack_add_scaled, xy, FB_OFFSET, ocw, s, 1.0, radius=4) == EINVAL, s
                assert code(ctx.stack_add_surfaces_scaled, surf, 4, s, 3.0) == EINVAL, s
                assert code(ctx.stack_layer_shift, s) == EINVAL, s
            for w in (0.0, -1.0, float("nan"), float("inf")):
                assert code(ctx.stack_add_scaled, xy, FB_OFFSET, ocw, 1.0, w, radius=4) == EINVAL, w
                assert code(ctx.stack_add_surfaces_scaled, surf, 4, 1.0, w) == EINVAL, w
            for Rl in (0, 48):
                assert code(ctx.stack_add_scaled, xy, FB_OFFSET, ocw, 1.0, 3.0, radius=Rl) == EINVAL, Rl
                assert code(ctx.stack_add_surfaces_scaled, np.zeros((n, (2 * Rl + 1) ** 2), np.float32), Rl, 1.0, 3.0) == EINVAL, Rl
            assert api.wide_max_radius(40) == 39
            assert code(ctx.stack_add_scaled, xy, FB_OFFSET, 40, 1.0, 3.0, radius=40) == EINVAL
            assert code(ctx.stack_add_scaled, xy, FB_OFFSET, 8, 1.0, 3.0, radius=4) == EINVAL              # ocw 8
            with pytest.raises(ValueError, match="pass a radius explicitly"):
                ctx.stack_add_scaled(xy, FB_OFFSET, 40, 10.0, 3.0)                                     # wants 41 > 39
            assert code(ctx.stack_add_scaled, xy[:-1], FB_OFFSET, ocw, 1.0, 3.0, radius=4) == EINVAL       # N differs
            assert code(ctx.stack_add_surfaces_scaled, surf[:-1], 4, 1.0, 3.0) == EINVAL
            assert code(ctx.stack_add_scaled, xy, (300, 0), ocw, 2.0, 3.0) == EBOUNDS                  # a box that leaves the zero border
            assert ctx.stack_info() == (n, radius, 1) and ctx.stack_weighted() == weighted
            same_bytes(ctx.stack_finish(3, 1, surface=True), before, f"after the refusals (weighted {weighted})")
        assert np.isfinite(before[0][:, 0]).sum() >= 20
        # |scale x shift| >= 2^30
        far = shift.copy()
        far[7] = (2 ** 25, -(2 ** 24))
        ctx.stack_begin(n, radius, far)
        ctx.stack_add_surfaces(np.full((n, 81), 0.25, np.float32))
        before = ctx.stack_finish(3, 1, surface=True)
        assert code(ctx.stack_add_surfaces_scaled, surf, 4, 32.0, 3.0) == EINVAL                      # 2^30 exactly
        assert code(ctx.stack_add_scaled, xy, FB_OFFSET, ocw, 64.0, 3.0, radius=4) == EINVAL
        assert code(ctx.stack_layer_shift, 32.0) == EINVAL
        assert ctx.stack_layer_shift(16.0)[7].tolist() == [2 ** 29, -(2 ** 28)]
        assert not ctx.stack_weighted() and ctx.stack_info() == (n, radius, 1)
        same_bytes(ctx.stack_finish(3, 1, surface=True), before, "after |scale x shift| >= 2^30")


# ---- 8. the _dev entries ----
def test_dev_entries_on_a_stream(api):
    import hipmem
    from hipmem import DevArray
    ocw, radius, npeaks = 7, 6, 3
    i0, i1, _ = class_pair("float")
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n, NC = xy.shape[0], (2 * radius + 1) ** 2
    Rx = 5
    extra = (np.random.default_rng(3).random((n, (2 * Rx + 1) ** 2)) - 0.3).astype(np.float32)
    extra_refused = np.arange(n) % 5 == 0
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add_scaled(xy, FB_OFFSET, ocw, 2.5)                     # layer radius 16: the wide kernel
        ctx.stack_add_surfaces_scaled(extra, Rx, 0.7, 2.0, refused=extra_refused)
        ctx.stack_add_scaled(xy, (2, -1), ocw, 0.5, 0.5, swap=True)
        want = ctx.stack_finish(npeaks, 2, surface=True)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        d_xy = DevArray(src=xy)
        # an unaligned caller's array: the surfaces start 4 bytes into the allocation
        d_extra = DevArray(src=np.concatenate([np.zeros(1, np.float32), extra.ravel()]))
        d_ref = DevArray(src=extra_refused.astype(np.uint8))
        d_out, d_cand = DevArray((n, 8), np.float32), DevArray((npeaks, n, 3), np.float32)
        d_surf, d_count = DevArray((n, NC), np.float32), DevArray((n,), np.uint16)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add_scaled_dev(d_xy.ptr, n, FB_OFFSET, ocw, 2.5, stream=st.value)
        ctx.stack_add_surfaces_scaled_dev(d_extra.ptr + 4, n, Rx, 0.7, 2.0, d_refused=d_ref.ptr, stream=st.value)
        ctx.stack_add_scaled_dev(d_xy.ptr, n, (2, -1), ocw, 0.5, 0.5, stream=st.value, swap=True)
        ctx.stack_finish_dev(npeaks, 2, d_out.ptr, d_cand=d_cand.ptr, d_surf=d_surf.ptr, d_count=d_count.ptr, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.stack_info() == (n, radius, 3) and ctx.stack_weighted()
        assert_bits_equal(d_out.numpy(), want[0], "_dev: record")
        assert_bits_equal(d_cand.numpy(), want[1], "_dev: candidates")
        assert np.array_equal(d_count.numpy(), want[2])
        assert_bits_equal(d_surf.numpy(), want[3], "_dev: mean surface")
        assert hipmem._hip.hipStreamDestroy(st) == 0
    assert np.isfinite(want[0][:, 0]).sum() >= 5


# ---- 9. the series over six time baselines ----
def test_the_series_on_the_device(api):
    """tests/test_stack_scaled_cpu.py's series through the device: the same counts"""
    xy, shift = scaled_series_points()
    n = xy.shape[0]
    per_layer = []
    with api.Context(0) as ctx, api.Context(0) as plain:
        ctx.stack_begin(n, SCALED_R, shift)
        plain.stack_begin(n, SCALED_R, shift)
        for s, i0, i1 in scaled_series_pairs():
            ctx.set_images(i0, i1)
            plain.set_images(i0, i1)
            Rl = api.stack_layer_radius(SCALED_R, s)
            rec = ctx.match_ncc_wide(xy, FB_OFFSET, SCALED_OCW, Rl, 0, shift=ctx.stack_layer_shift(s))[0]
            per_layer.append(int(misplaced(rec, layer_truth(s)).sum()))
            ctx.stack_add_scaled(xy, FB_OFFSET, SCALED_OCW, s)
            plain.stack_add(xy, FB_OFFSET, SCALED_OCW)
        rec = ctx.stack_finish()[0]
        stacked = int(misplaced(rec, SCALED_MOTION).sum())
        unscaled = int(misplaced(plain.stack_finish()[0], SCALED_MOTION).sum())
    print(f"device: misplaced per layer {per_layer}, scaled stack {stacked}, unscaled stack {unscaled}")
    assert (per_layer, stacked, unscaled) == SCALED_COUNTS and rec[56, 2] == -4
