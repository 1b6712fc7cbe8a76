"""GPU: scaled stack layers at any chip size and layer radius, resampled in the matrix-core search's own tail
(mimc3_stack_add_scaled_fused, mimc3_stack_add_scaled_fused_dev; stack_acc_scaled in stack_acc.h).

By definition a fused scaled layer is match_ncc_wide_planes(mode 0, surface, shift = the layer shift, radius = the layer's) +
stack_add_surfaces_scaled(surface, refused_of(record), layer radius, scale, weight): every comparison below is byte for byte on
everything stack_finish(k, min_count, surface=True) returns, for (k, min_count) in (4, 1), (0, 2), (8, 3) -- the mean exposes sum and
wsum (every case is weighted by its second layer at the latest; the unweighted state is compared in the scale-1 and at-the-six tests),
the min_count steps expose cnt, count exposes lay.  Fixtures and the case table: tests/stack_scaled_fused_common.py, qualified without a
device in tests/test_stack_scaled_fused_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import stack_fused_common as sf
import stack_scaled_fused_common as sc
from conftest import assert_bits_equal
from full_any_common import full_any
from full_fb_common import FB_OFFSET, class_pair, fb_points
from stack_common import refused_of
from stack_scaled_common import NumpyScaledStack, layer_radius, layer_shift

pytestmark = pytest.mark.gpu

EINVAL, EBOUNDS, ESTATE = -1, -2, -5


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def last_error(api):
    return api._lib.mimc3_last_error().decode(errors="replace")


def set_pair(api, ctx, f):
    """the fixture's pair on the context; "ddx": the 8-bit pair, d/dx-filtered on the device (a scaled-integer pair)"""
    ctx.set_images(f["i0"], f["i1"])
    if f["kind"] == "ddx":
        ctx.filter_images(api.CLI_KERNELS[0])


def chain_layer(ctx, xy, off, shift, ocw, swap, scale, weight, layer_r):
    """the definition's two calls"""
    rec, _, surf = ctx.match_ncc_wide_planes(xy, off, ocw, layer_r, 0, shift=layer_shift(shift, scale), swap=swap, mode=0, surface=True)
    ctx.stack_add_surfaces_scaled(surf, layer_r, scale, weight, refused_of(rec))
    return rec


def compare(got, want, what):
    for a, b, (k, mc) in zip(got, want, sf.FINISHES):
        sf.same_bytes(a, b, f"{what} npeaks {k} min_count {mc}")


def compare_with_numpy(got, ref, what):
    for (rec, cand, count, mean), (k, mc) in zip(got, sf.FINISHES):
        w_rec, w_cand, w_lay, w_mean = ref.finish(k, mc)
        tag = f"{what} npeaks {k} min_count {mc} vs NumpyScaledStack over the oracle's surfaces"
        assert count.dtype == np.uint16 and np.array_equal(count, w_lay), tag + ": count"
        assert_bits_equal(mean, w_mean, tag + ": mean surface")
        assert_bits_equal(rec, w_rec, tag + ": record")
        if k:
            assert_bits_equal(cand, w_cand, tag + ": candidates")


def fused_vs_chain(api, case, nulls="placed", npts=None):
    f = sc.fixture(case, nulls)
    kind, ocw, R = case[0], case[1], case[2]
    n = f["c"].n if npts is None else npts
    xy, shift, off = np.ascontiguousarray(f["xy"][:n]), np.ascontiguousarray(f["shift"][:n]), f["off"]
    layers = sc.layers_of(case)
    with api.Context(0) as ctx:
        set_pair(api, ctx, f)
        ctx.stack_begin_wide(n, R, shift)
        weighted = False
        for k, (o, swap, s, w, rl) in enumerate(layers):
            assert ctx.stack_fused_max_radius(o) == sf.max_radius(kind, o, api) >= rl
            ctx.stack_add_scaled_fused(xy, off, o, s, w, radius=rl, swap=swap)
            weighted = weighted or w != 1.0
            assert ctx.last_path() == sf.path_of(kind, rl), f["what"]
            assert ctx.stack_info() == (n, R, k + 1) and ctx.stack_weighted() == weighted
        got = sf.finishes(ctx)
        ctx.stack_begin_wide(n, R, shift)
        assert not ctx.stack_weighted()
        recs = [chain_layer(ctx, xy, off, shift, *layer) for layer in layers]
        assert ctx.stack_weighted() == weighted
        want = sf.finishes(ctx)
    compare(got, want, f"{f['what']} n {n}: stack_add_scaled_fused vs the two-call chain,")
    return got, recs, f


# ---- 1. fused vs chain, every case of the table ----
@pytest.mark.parametrize("case", sc.CASES + (sc.ALL_KINDS_CASE,), ids=sc.case_id)
def test_fused_scaled_layers_are_the_chain_s(api, case):
    got, recs, f = fused_vs_chain(api, case)
    count, mean = got[0][2], got[0][3]
    assert recs[0][sf.REFUSED, 2] == -3 and count[sf.REFUSED] < 3 and (np.delete(count, sf.REFUSED) == 3).all()
    kinds = sc.cell_kinds(f["shift"], case[2], case[3], case[5]).reshape(f["c"].n, -1)
    clean = np.delete(np.arange(f["c"].n), sf.BOX_ONLY + sf.CHIP_ONLY + sf.BOTH + (sf.REFUSED,))
    # (the comparison is not one of NaNs alone: on a clean point every cell that lands inside the first layer has a mean)
    assert (kinds[clean] > 0).sum() >= 17 and np.isfinite(mean[clean][kinds[clean] > 0]).all()


# ---- 2. against NumpyScaledStack over the CPU oracle's surfaces ----
@pytest.mark.parametrize("case", sc.ORACLE_CASES, ids=sc.case_id)
def test_fused_scaled_stack_is_the_definition_s(api, case):
    f = sc.fixture(case)
    ref = sc.oracle_stack(f, case)
    with api.Context(0) as ctx:
        set_pair(api, ctx, f)
        ctx.stack_begin_wide(f["c"].n, f["R"], f["shift"])
        for o, swap, s, w, rl in sc.layers_of(case):
            ctx.stack_add_scaled_fused(f["xy"], f["off"], o, s, w, radius=rl, swap=swap)
        assert ctx.stack_weighted() == ref.weighted
        got = sf.finishes(ctx)
    compare_with_numpy(got, ref, f["what"])


# ---- 3. at the six chip sizes within wide_max_radius: stack_add_scaled's bytes, weighted or not ----
@pytest.mark.parametrize("case", sc.SIX_CASES, ids=sc.case_id)
def test_at_the_six_it_is_stack_add_scaled(api, case):
    kind, ocw, R, scale, weight, layer_r, ocw2 = case
    f = sc.fixture(case)
    n, xy, shift, off = f["c"].n, f["xy"], f["shift"], f["off"]
    layers = [(o if o in sf.SIX else ocw, swap, s, weight, rl) for o, swap, s, w, rl in sc.layers_of(case)]     # (one weight: unweighted at 1)
    with api.Context(0) as ctx:
        set_pair(api, ctx, f)
        got = {}
        for add in ("stack_add_scaled_fused", "stack_add_scaled"):
            ctx.stack_begin_wide(n, R, shift)
            for o, swap, s, w, rl in layers:
                assert rl <= api.wide_max_radius(o)
                getattr(ctx, add)(xy, off, o, s, w, radius=rl, swap=swap)
                if add == "stack_add_scaled_fused":
                    assert ctx.last_path() == sf.path_of(kind, rl)
            assert ctx.stack_weighted() == (weight != 1.0)
            got[add] = sf.finishes(ctx)
    compare(got["stack_add_scaled_fused"], got["stack_add_scaled"], f"{f['what']}: stack_add_scaled_fused vs stack_add_scaled,")
    assert np.isfinite(got["stack_add_scaled_fused"][0][3]).sum() >= 17


# ---- 4. scale 1, weight 1, the stack's radius: stack_add_fused's bytes ----
@pytest.mark.parametrize("case", (sc.CASES[0], ("dn12", 16, 20, 1.0, 1.0, 20, 15)), ids=sc.case_id)
def test_scale_one_weight_one_is_stack_add_fused(api, case):
    kind, ocw, R, scale, weight, layer_r, ocw2 = case
    f = sc.fixture(case)
    n, xy, shift, off = f["c"].n, f["xy"], f["shift"], f["off"]
    with api.Context(0) as ctx:
        set_pair(api, ctx, f)
        ctx.stack_begin_wide(n, R, shift)
        for o, swap in ((ocw, False), (ocw, True), (ocw2, False)):
            ctx.stack_add_scaled_fused(xy, off, o, 1.0, 1.0, swap=swap)                  # (radius None: stack_layer_radius(R, 1) = R)
            assert ctx.last_path() == sf.path_of(kind, R)
        assert not ctx.stack_weighted()
        got = sf.finishes(ctx)
        ctx.stack_begin_wide(n, R, shift)
        for o, swap in ((ocw, False), (ocw, True), (ocw2, False)):
            ctx.stack_add_fused(xy, off, o, swap=swap)
        want = sf.finishes(ctx)
    compare(got, want, f"{f['what']}: scale 1, weight 1 vs stack_add_fused,")
    assert (got[0][0][:, 2] >= -1).sum() >= 20


# ---- 5. every kind of add in one stack: the numpy definition over the oracle's surfaces ----
def test_mixed_stack_is_the_definition_s(api):
    case = sc.CASES[1]                                                   # u8, ocw 10, R 4, scale 2, layer R 9
    kind, ocw, R, scale, weight, layer_r, ocw2 = case
    f = sc.fixture(case)
    n, xy, shift, off = f["c"].n, f["xy"], f["shift"], f["off"]
    s4, r4 = 0.5, layer_radius(R, 0.5)
    rec1, _, surf1, _ = full_any(f["i0"], f["i1"], xy, off, ocw, R, 0, shift=shift)
    rec2, _, surf2, _ = full_any(f["i0"], f["i1"], xy, off, ocw, layer_r, 0, shift=layer_shift(shift, scale))
    rec3, _, surf3, _ = full_any(f["i0"], f["i1"], xy, off, ocw2, R, 0, shift=shift, swap=True)
    rec4, _, surf4, _ = full_any(f["i0"], f["i1"], xy, off, ocw, r4, 0, shift=layer_shift(shift, s4), swap=True)
    ref = NumpyScaledStack(n, R, shift).add(surf1, refused_of(rec1)).add_scaled(surf2, layer_r, scale, 1.0, refused_of(rec2))
    ref.add(surf3, refused_of(rec3))
    assert not ref.weighted
    cnt3 = ref.cnt.copy()
    ref.add_scaled(surf4, r4, s4, 0.3, refused_of(rec4))
    fin4 = np.isfinite(sc.resample_value(surf4, r4, shift, R, s4))
    assert ref.weighted and np.array_equal(ref.wsum, cnt3 + 0.3 * fin4)   # wsum starts from cnt on the fourth add
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin(n, R, shift)
        ctx.stack_add_fused(xy, off, ocw)
        ctx.stack_add_scaled_fused(xy, off, ocw, scale, 1.0, radius=layer_r)
        assert ctx.last_path() == "u8_mfma_chip" and not ctx.stack_weighted()
        ctx.stack_add_surfaces(surf3, refused_of(rec3))
        assert not ctx.stack_weighted()
        ctx.stack_add_scaled_fused(xy, off, ocw, s4, 0.3, swap=True)
        assert ctx.stack_weighted() and ctx.stack_info() == (n, R, 4) and ctx.last_path() == "u8_mfma_chip"
        got = sf.finishes(ctx)
    compare_with_numpy(got, ref, "the mixed stack")


# ---- 6. every point dirty (the masked form alone), every point refused ----
@pytest.mark.parametrize("case", (sc.CASES[1], sc.CASES[2], sc.CASES[10], sc.CASES[11]), ids=sc.case_id)
def test_every_point_dirty_and_every_point_refused(api, case):
    got, recs, f = fused_vs_chain(api, case, nulls="all")
    assert (got[0][2] == 3).all() and np.isfinite(got[0][3]).any(axis=1).sum() >= 20
    kind, ocw, R, scale, weight, layer_r, _ = case
    f = sc.fixture(case, "refused")
    n = f["c"].n
    with api.Context(0) as ctx:
        set_pair(api, ctx, f)
        ctx.stack_begin_wide(n, R, f["shift"])
        for _ in range(2):
            ctx.stack_add_scaled_fused(f["xy"], f["off"], ocw, scale, weight, radius=layer_r)
        assert ctx.last_path() == sf.path_of(kind, layer_r) and ctx.stack_info() == (n, R, 2)      # layers counts ...
        rec, _, count, mean = ctx.stack_finish(0, 1, surface=True)
    assert (count == 0).all() and (rec[:, 2] == -3).all() and np.isnan(mean).all()                 # ... lay stays 0


@pytest.mark.parametrize("case", (sc.CASES[1], sc.CASES[2], sc.CASES[11]), ids=sc.case_id)
@pytest.mark.parametrize("npts", (1, 13))
def test_grids_that_are_no_multiple_of_eight(api, case, npts):
    fused_vs_chain(api, case, npts=npts)


# ---- 7. the _dev entry ----
@pytest.mark.parametrize("case", (sc.CASES[1], sc.CASES[2], sc.CASES[10], sc.CASES[11]), ids=sc.case_id)
def test_dev_entry_on_a_stream_of_its_own(api, case):
    import hipmem
    from hipmem import DevArray
    kind, ocw, R, scale, weight, layer_r, _ = case
    f = sc.fixture(case)
    n, xy, shift, off = f["c"].n, f["xy"], f["shift"], f["off"]
    out = 9                                                              # a clean point
    bad = xy.copy()
    bad[out, 2] = 2.0                                                    # its chip leaves the image: only the _dev entry takes the row
    s2, w2, r2 = sc.second_layer(case)
    with api.Context(0) as ctx:
        set_pair(api, ctx, f)
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_scaled_fused(xy, off, ocw, scale, weight, radius=layer_r)
        ctx.stack_add_scaled_fused(xy, off, ocw, s2, w2, radius=r2, swap=True)
        want = sf.finishes(ctx)
        with pytest.raises(api.Mimc3Error) as e:
            ctx.stack_add_scaled_fused(bad, off, ocw, scale, weight, radius=layer_r)
        assert e.value.code == EBOUNDS and ctx.stack_info() == (n, R, 2)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        d_xy, d_bad = DevArray(src=np.ascontiguousarray(xy)), DevArray(src=np.ascontiguousarray(bad))
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_scaled_fused_dev(d_xy.ptr, n, off, ocw, scale, weight, radius=layer_r, stream=st.value)
        ctx.stack_add_scaled_fused_dev(d_xy.ptr, n, off, ocw, s2, w2, radius=r2, stream=st.value, swap=True)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == sf.path_of(kind, r2) and ctx.stack_info() == (n, R, 2) and ctx.stack_weighted()
        compare(sf.finishes(ctx), want, f"{f['what']}: _dev on a stream of its own vs the host entry,")
        # the row whose chip leaves the image: the layer counts, its cells get nothing, every other point is the host entry's
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_scaled_fused_dev(d_bad.ptr, n, off, ocw, scale, weight, radius=layer_r, stream=st.value)
        ctx.stack_add_scaled_fused_dev(d_xy.ptr, n, off, ocw, s2, w2, radius=r2, stream=st.value, swap=True)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        rec1, _, count1, mean1 = ctx.stack_finish(4, 1, surface=True)
        rec2, _, count2, mean2 = ctx.stack_finish(0, 2, surface=True)
        assert hipmem._hip.hipStreamDestroy(st) == 0
    w1, w2_ = want[0], want[1]                                           # (npeaks 4, min_count 1), (0, 2)
    assert np.array_equal(count1, w1[2]) and count1[out] == 2            # the layer counts ...
    assert np.isnan(mean2[out]).all() and np.isfinite(mean1[out]).any()  # ... but no cell has two values: the bad row added none
    others = np.arange(n) != out
    assert mean1[others].tobytes() == w1[3][others].tobytes() and mean2[others].tobytes() == w2_[3][others].tobytes()
    assert rec2[others].tobytes() == w2_[0][others].tobytes()


# ---- 8. any other pair: not fused, the kernel of match_ncc_wide_planes(mode 0) through the layer scratch ----
def test_a_16_bit_pair_runs_the_chain_s_kernel_at_any_chip_size(api):
    i0, i1, _ = class_pair("dn16")
    R, ocw, scale, layer_r = 4, 10, 2.0, 9
    xy, shift = fb_points(ocw=ocw, radius=R)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        assert ctx.stack_fused_max_radius(ocw) == 15
        ctx.stack_begin(n, R, shift)
        for swap, w in ((False, 1.0), (True, 0.3)):
            ctx.stack_add_scaled_fused(xy, FB_OFFSET, ocw, scale, w, swap=swap)          # (radius None: stack_layer_radius(4, 2) = 9)
            assert ctx.last_path() == "f32g_chip"
        got = sf.finishes(ctx)
        ctx.stack_begin(n, R, shift)
        for swap, w in ((False, 1.0), (True, 0.3)):
            chain_layer(ctx, xy, FB_OFFSET, shift, ocw, swap, scale, w, layer_r)
            assert ctx.last_path() == "f32g_chip"
        want = sf.finishes(ctx)
        compare(got, want, "dn16 ocw 10 layer R 9: the fallback vs the chain,")
        assert (got[0][0][:, 2] >= -1).sum() >= 20
        # ... and beyond layer R 15 no kernel takes the chip size: refused, with the limit, the stack as it was
        code = api._lib.mimc3_stack_add_scaled_fused(ctx._h, xy, n, np.ascontiguousarray(FB_OFFSET, np.int32), ocw, 16, 0, scale, 0.3)
        assert code == EINVAL and "layer_R must be in 1..15" in last_error(api)
        with pytest.raises(ValueError):
            ctx.stack_add_scaled_fused(xy, FB_OFFSET, ocw, 4.0)                          # stack_layer_radius(4, 4) = 17 > 15
        assert ctx.stack_info() == (n, R, 2)
        compare(sf.finishes(ctx), want, "a refused add leaves the stack as it was,")


def test_a_16_bit_pair_at_the_six_is_stack_add_scaled(api):
    i0, i1, _ = class_pair("dn16")
    R, ocw, scale, layer_r = 8, 16, 2.5, 20
    xy, shift = fb_points(ocw=ocw, radius=R)
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        assert ctx.stack_fused_max_radius(ocw) == api.wide_max_radius(ocw) >= layer_r
        got = {}
        for add in ("stack_add_scaled_fused", "stack_add_scaled"):
            ctx.stack_begin(n, R, shift)
            for swap, w in ((False, 1.0), (True, 0.3)):
                getattr(ctx, add)(xy, FB_OFFSET, ocw, scale, w, radius=layer_r, swap=swap)
                assert ctx.last_path() == "f32g_wide"
            got[add] = sf.finishes(ctx)
    compare(got["stack_add_scaled_fused"], got["stack_add_scaled"], "dn16 ocw 16 layer R 20: the fallback vs stack_add_scaled,")
    assert np.isfinite(got["stack_add_scaled"][0][3]).any(axis=1).sum() >= 20


# ---- 9. refusals: the stack's bytes, stack_info and stack_weighted stay as they were ----
def test_refusals_leave_the_stack_untouched(api):
    from hipmem import DevArray
    case = sc.CASES[1]
    kind, ocw, R, scale, weight, layer_r, _ = case
    f = sc.fixture(case)
    n, xy, shift, off = f["c"].n, np.ascontiguousarray(f["xy"]), f["shift"], f["off"]
    call, dev = api._lib.mimc3_stack_add_scaled_fused, api._lib.mimc3_stack_add_scaled_fused_dev
    with api.Context(0) as ctx:
        ctx.stack_begin(n, R, shift)
        assert call(ctx._h, xy, n, off, ocw, layer_r, 0, scale, 1.0) == ESTATE           # no images
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin(0, R)
        assert call(ctx._h, xy, n, off, ocw, layer_r, 0, scale, 1.0) == ESTATE           # no stack
        ctx.stack_begin(n, R, shift)
        ctx.stack_add_scaled_fused(xy, off, ocw, scale, 1.0, radius=layer_r)
        assert not ctx.stack_weighted()
        want = sf.finishes(ctx)
        d_xy = DevArray(src=xy)
        # those of mimc3_stack_add_fused
        assert call(ctx._h, np.ascontiguousarray(xy[:5]), 5, off, ocw, layer_r, 0, scale, 1.0) == EINVAL     # N differs from the stack's
        assert dev(ctx._h, d_xy.ptr, 5, 1, -1, ocw, layer_r, 0, scale, 1.0, None) == EINVAL
        for o in (0, 81, -3):
            assert call(ctx._h, xy, n, off, o, layer_r, 0, scale, 1.0) == EINVAL
            assert dev(ctx._h, d_xy.ptr, n, 1, -1, o, layer_r, 0, scale, 1.0, None) == EINVAL
        assert dev(ctx._h, None, n, 1, -1, ocw, layer_r, 0, scale, 1.0, None) == EINVAL  # null pointers
        assert dev(None, d_xy.ptr, n, 1, -1, ocw, layer_r, 0, scale, 1.0, None) == EINVAL
        assert call(ctx._h, xy, 0, off, ocw, layer_r, 0, scale, 1.0) == EINVAL
        # those of the scaled adds: scale, weight, layer_R (with the limit), each with a weight that would make the stack weighted
        for s in (0.0, 1.0 / 128, 65.0, -2.0, float("nan"), float("inf")):
            assert call(ctx._h, xy, n, off, ocw, layer_r, 0, s, 0.3) == EINVAL and "scale" in last_error(api)
            assert dev(ctx._h, d_xy.ptr, n, 1, -1, ocw, layer_r, 0, s, 0.3, None) == EINVAL
        for w in (0.0, -1.0, float("nan"), float("inf")):
            assert call(ctx._h, xy, n, off, ocw, layer_r, 0, scale, w) == EINVAL and "weight" in last_error(api)
            assert dev(ctx._h, d_xy.ptr, n, 1, -1, ocw, layer_r, 0, scale, w, None) == EINVAL
        lim = ctx.stack_fused_max_radius(ocw)
        assert lim == 47
        for rl in (0, -1, lim + 1, 95):
            assert call(ctx._h, xy, n, off, ocw, rl, 0, scale, 0.3) == EINVAL and f"layer_R must be in 1..{lim}" in last_error(api)
            assert dev(ctx._h, d_xy.ptr, n, 1, -1, ocw, rl, 0, scale, 0.3, None) == EINVAL
        assert not ctx.stack_weighted()                                  # (the w != 1 calls that failed on layer_R left it unweighted)
        with pytest.raises(ValueError):
            ctx.stack_add_scaled_fused(xy, off, ocw, 16.0)               # stack_layer_radius(4, 16) = 65 > 47: the Python entry says so
        # the host entry's bounds, on the chips and on the LAYER's box
        bad = xy.copy()
        bad[3, 2] = 3.0
        assert call(ctx._h, bad, n, off, ocw, layer_r, 0, scale, 0.3) == EBOUNDS          # a chip that leaves the image
        assert call(ctx._h, xy, n, np.array([700, 0], np.int32), ocw, layer_r, 0, scale, 0.3) == EBOUNDS     # a box that leaves the zero border
        H, W = f["i0"].shape
        reach = int((xy[:, 2].astype(np.int64) + f["lsh"][:, 0]).max()) + ocw + layer_r                # the rightmost box edge at offset 0
        edge = np.array([W + 256 - reach, int(off[1])], np.int32)
        assert call(ctx._h, xy, n, edge, ocw, layer_r, 0, scale, 0.3) == EBOUNDS          # the layer's box ends one pixel beyond the border ...
        edge[0] -= 1
        assert ctx.stack_info() == (n, R, 1) and not ctx.stack_weighted()
        compare(sf.finishes(ctx), want, "a refused add leaves the stack as it was,")
        assert call(ctx._h, xy, n, edge, ocw, layer_r, 0, scale, 1.0) == 0                # ... and is taken where it ends on it
        assert ctx.stack_info() == (n, R, 2)
        # |scale x shift| >= 2^30
        far = shift.copy()
        far[5, 1] = -(1 << 25)
        ctx.stack_begin(n, R, far)
        before = sf.finishes(ctx)
        assert call(ctx._h, xy, n, off, ocw, 47, 0, 32.0, 0.3) == EINVAL and "2^30" in last_error(api)
        assert dev(ctx._h, d_xy.ptr, n, 1, -1, ocw, 47, 0, 32.0, 0.3, None) == EINVAL
        assert ctx.stack_info() == (n, R, 0) and not ctx.stack_weighted()
        compare(sf.finishes(ctx), before, "a refused add leaves the empty stack as it was,")


def test_a_full_stack_refuses_the_layer(api):
    """65,535 layers of one point's 3 x 3 surface, then the fused scaled add: MIMC3_ESTATE, the stack as it was"""
    from hipmem import DevArray
    f = sc.fixture(sc.CASES[1])
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
        assert api._lib.mimc3_stack_add_scaled_fused(ctx._h, xy, 1, off, 10, 3, 0, 2.0, 0.3) == ESTATE
        assert ctx.stack_info() == (1, 1, 65535) and not ctx.stack_weighted()
        sf.same_bytes(ctx.stack_finish(0, 1, surface=True), before, "a full stack")
