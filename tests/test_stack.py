"""GPU: NCC stacking (mimc3_stack_*, stack_kernel.hip).

Every comparison is bit for bit (NaNs by position).  A stack of one layer returns the bytes of match_ncc_full_any(mode=1) on every pixel
class; a stack of several layers returns what the numpy definition (tests/stack_common.py: sequential f64 adds in layer order, the
counts, the mean, then the oracle's tail in the device's SNR order) makes of the same layers' surfaces, which the existing
match_ncc_full_any(..., surface=True) serves; crafted surfaces exercise ties, plateaus, borders, min_count, Inf and the f64 order; the
accumulator survives finish, set_images and refused calls; the chunk edge; the _dev entries on a stream of their own."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_fb_common import FB_OFFSET, class_pair, fb_pair, fb_points
from stack_common import SHAPES, NumpyStack, refused_of

pytestmark = pytest.mark.gpu

NPEAKS = (0, 3, 8)
EINVAL, EBOUNDS, ESTATE = -1, -2, -5


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def layer_of(ctx, xy, offset, ocw, radius, shift, swap=False):
    """One layer as the existing entry serves it -> (surfaces, refused)"""
    rec, _, surf = ctx.match_ncc_full_any(xy, offset, ocw, radius, 0, shift=shift, swap=swap, mode=1, surface=True)
    return surf, refused_of(rec)


def check_finish(ctx, ref, what, npeaks_list=NPEAKS, min_counts=(1,)):
    """ctx's stack against the numpy stack `ref`: record, candidates, count and mean surface"""
    assert ctx.stack_info() == (ref.n, ref.radius, ref.layers), what
    for mc in min_counts:
        for npeaks in npeaks_list:
            rec, cand, count, surf = ctx.stack_finish(npeaks, mc, surface=True)
            w_rec, w_cand, w_lay, w_mean = ref.finish(npeaks, mc)
            tag = f"{what}: npeaks {npeaks} min_count {mc}"
            assert count.dtype == np.uint16 and np.array_equal(count, w_lay), tag + ": count"
            assert_bits_equal(surf, w_mean, tag + ": mean surface")
            assert_bits_equal(rec, w_rec, tag + ": record")
            assert (cand is None) == (npeaks == 0)
            if npeaks:
                assert_bits_equal(cand, w_cand, tag + ": candidates")
            rec2, cand2, count2 = ctx.stack_finish(npeaks, mc)
            assert_bits_equal(rec2, rec, tag + ": record without the surface")
            assert np.array_equal(count2, count)
    return rec


# ---- 1. one layer is the search ----
@pytest.mark.parametrize("ocw,radius", SHAPES)
@pytest.mark.parametrize("kind", ("u8", "dn12", "dn16", "float"))
def test_one_layer_equals_match_ncc_full_any(api, kind, ocw, radius):
    i0, i1, _ = class_pair(kind)
    xy, shift = fb_points(ocw=ocw, radius=radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for pts, sh_all in ((xy, shift), (xy[:1], shift[:1])):           # 60 points, and N = 1
            for sh in (sh_all, None):
                ctx.stack_begin(pts.shape[0], radius, sh)
                ctx.stack_add(pts, FB_OFFSET, ocw)
                assert ctx.last_path() == "f32g_full"
                assert ctx.stack_info() == (pts.shape[0], radius, 1)
                for npeaks in NPEAKS:
                    what = f"{kind} ocw {ocw} R {radius} N {pts.shape[0]} shift {sh is not None} npeaks {npeaks}"
                    rec, cand, count, surf = ctx.stack_finish(npeaks, 1, surface=True)
                    w = ctx.match_ncc_full_any(pts, FB_OFFSET, ocw, radius, npeaks, shift=sh, mode=1, surface=True)
                    assert_bits_equal(rec, w[0], what + ": record")
                    assert_bits_equal(surf, w[2], what + ": surface")
                    assert np.array_equal(count, (~refused_of(w[0])).astype(np.uint16)), what
                    if npeaks:
                        assert_bits_equal(cand, w[1], what + ": candidates")
                if pts.shape[0] > 1:
                    assert (rec[:, 2] >= -1).sum() >= 20                  # (the comparison is not one of NaNs alone)


# ---- 2. three layers ----
def null_box(img, xy, shift, point, ocw, radius, cols):
    """Null (0) the columns `cols` (relative to the box's left edge) of point's search box in img, all its rows"""
    cu = int(xy[point, 2]) + FB_OFFSET[0] + shift[point, 0]
    cv = int(xy[point, 3]) + FB_OFFSET[1] + shift[point, 1]
    h = ocw + radius
    img[cv - h:cv + h + 1, cu - h + cols[0]:cu - h + cols[1]] = 0


def three_pairs(xy, shift, ocw=7, radius=4):
    """Three 8-bit pairs with different nulls.  The left 16 of the 23 box columns of point 20 are null in image 1 of layers 0 and 1, those
    of point 30 in layer 0: their cells su = -4, -3 have no pixel pair there (NaN) but the point stays valid (70 % < 80 %).  The chip
    of point 40 is null in layer 1 (refused there), the chip of point 41 in all three."""
    pairs = []
    for k in range(3):
        i0, i1 = fb_pair(seed=41 + k)
        if k < 2:
            null_box(i1, xy, shift, 20, ocw, radius, (0, 16))
        if k == 0:
            null_box(i1, xy, shift, 30, ocw, radius, (0, 16))
        for point in (40, 41) if k == 1 else (41,):
            u, v = int(xy[point, 2]), int(xy[point, 3])
            i0[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1] = 0
        pairs.append((i0, i1))
    return pairs


def test_three_layers_with_different_nulls(api):
    ocw, radius = 7, 4
    xy, shift = fb_points(ocw=ocw, radius=radius)
    ref = NumpyStack(xy.shape[0], radius, shift)
    with api.Context(0) as ctx:
        ctx.stack_begin(xy.shape[0], radius, shift)
        for i0, i1 in three_pairs(xy, shift):
            ctx.set_images(i0, i1)                                       # (a new pair between the adds: the stack stays)
            ref.add(*layer_of(ctx, xy, FB_OFFSET, ocw, radius, shift))
            ctx.stack_add(xy, FB_OFFSET, ocw)
        # the fixture does what it is for
        assert ref.lay[40] == 2 and ref.lay[41] == 0 and ref.lay[20] == 3
        assert (ref.cnt[20] == 1).any() and (ref.cnt[20] == 3).any() and (ref.cnt[30] == 2).any()
        rec = check_finish(ctx, ref, "three pairs", min_counts=(1, 2, 3))
        assert rec[41, 2] == -3 and rec[40, 2] != -3


def test_chip_sizes_and_a_swapped_layer_in_one_stack(api):
    radius = 6
    xy, shift = fb_points(ocw=30, radius=radius)
    i0, i1, _ = class_pair("float")
    ref = NumpyStack(xy.shape[0], radius, shift)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(xy.shape[0], radius, shift)
        for ocw, swap in ((15, False), (16, False), (30, False), (16, True)):
            ref.add(*layer_of(ctx, xy, FB_OFFSET, ocw, radius, shift, swap=swap))
            ctx.stack_add(xy, FB_OFFSET, ocw, swap=swap)
        check_finish(ctx, ref, "ocw 15 / 16 / 30 and a swapped layer", min_counts=(1, 4))


# ---- 3. crafted surfaces, and 4. finish leaves the accumulator alone ----
def crafted_layers(radius, nlayers=7, seed=9):
    """Eight points, seven layers -> (list of surfaces float32[8][cells], refused bool[8]).
    0  seven layers of non-dyadic values: the f64 sums depend on the order of the additions;
    1  exact ties of the mean: a cell with 0.5 and 0.25 against two cells with 0.375 twice, everything else lower: first-wins k decides;
    2  a plateau: every cell the same;
    3  the best mean on the border (k = 0), lower interior peaks: -4, the candidates are the interior ones;
    4  finite in layer 0 alone: every cell is below min_count 2;
    5  the centre is the peak; one cell of its 3x3 block is NaN in every layer, another finite in layer 0 alone;
    6  +Inf and -Inf cells in several layers: ignored, not summed;
    7  as point 0, refused in every layer."""
    S = 2 * radius + 1
    NC = S * S
    rng = np.random.default_rng(seed + radius)
    ctr = radius * S + radius
    layers = []
    for k in range(nlayers):
        s = (rng.random((8, NC)) * 0.9 - 0.3).astype(np.float32)
        # 1: ties (R 1 has one interior cell: the tie is then between the centre and two border cells)
        s[1] = np.nan
        if k < 2:
            s[1] = 0.1
            a, b, c = (ctr, 1, NC - 1) if radius == 1 else (ctr, ctr - S - 1, ctr + 2 * S)
            s[1, a] = (0.5, 0.25)[k]
            s[1, b] = s[1, c] = 0.375
        s[2] = 0.3 if k < 2 else np.nan
        s[3] *= 0.5
        s[3, 0] = 0.9
        if k > 0:
            s[4] = np.nan
        s[5] = np.abs(s[5]) * 0.5
        s[5, ctr] = 0.8
        s[5, ctr - 1] = np.nan
        if k > 0:
            s[5, ctr + S] = np.nan
        inf_cells = rng.choice(NC, 3, replace=False)
        if k % 2 == 0:
            s[6, inf_cells[0]] = np.inf
            s[6, inf_cells[1]] = -np.inf
        if k == 1:
            s[6, ctr] = np.inf
        layers.append(np.ascontiguousarray(s))
    refused = np.zeros(8, bool)
    refused[7] = True
    return layers, refused


@pytest.mark.parametrize("radius", (1, 2, 15))
def test_crafted_surfaces(api, radius):
    layers, refused = crafted_layers(radius)
    ref = NumpyStack(8, radius)
    with api.Context(0) as ctx:                                          # (no images: add_surfaces needs none)
        ctx.stack_begin(8, radius)
        check_finish(ctx, ref, f"R {radius}: an empty stack", npeaks_list=(0, 3))
        for k, s in enumerate(layers[:-1]):
            ref.add(s, refused)
            ctx.stack_add_surfaces(s, refused)
            if k in (0, 1):
                check_finish(ctx, ref, f"R {radius}: {k + 1} layers", min_counts=(1, 2))
        rec = check_finish(ctx, ref, f"R {radius}: six layers", min_counts=(1, 2, 6))      # finishes several times: the same bytes
        assert rec[7, 2] == -3 and rec[3, 2] == -4 and rec[4, 2] == -2
        ref.add(layers[-1], refused)
        ctx.stack_add_surfaces(layers[-1], refused)                      # finish, add, finish: the definition on all layers
        rec = check_finish(ctx, ref, f"R {radius}: seven layers", min_counts=(1, 2, 7))
        # what the crafted points are for, at min_count 1 (rec is of min_count 7's last call: take min_count 1 again)
        rec, cand, count = ctx.stack_finish(8, 1)
        S = 2 * radius + 1
        assert count.tolist() == [7] * 7 + [0]
        assert rec[3, 2] == -4 and (cand[0, 3, 2] > -1) == (radius > 1) and rec[7, 2] == -3 and (cand[:, 7, 2] == -3).all()
        assert rec[1, 2] == (-4 if radius == 1 else np.float32(0.375)) and rec[2, 2] == -4      # the tie and the plateau: the lowest k
        assert rec[5, 2] == np.float32(0.8) and np.isnan(rec[5, 0])      # a NaN inside the 3x3 block: the peak stands, the fit is NaN
        assert np.isfinite(rec[6, 2]) or rec[6, 2] in (-2, -4)
        assert np.isfinite(ctx.stack_finish(0, 1, surface=True)[3][6]).all()     # Inf cells: no trace in the mean
        # every point refused
        ctx.stack_begin(8, radius)
        ctx.stack_add_surfaces(layers[0], np.ones(8, bool))
        rec, cand, count = ctx.stack_finish(2, 1)
        assert (rec[:, 2] == -3).all() and (cand[:, :, 2] == -3).all() and np.isnan(rec[:, [0, 1, 3, 4, 5, 6, 7]]).all() and not count.any()


# ---- 5. the chunk edge ----
def test_chunk_edge(api):
    n = api.STACK_CHUNK + 1
    i0, i1 = fb_pair()
    base, _ = fb_points(ocw=7, radius=1)
    xy = np.ascontiguousarray(base[np.arange(n) % 56])                   # the grid's 56 points over and over, plus one
    xy[:, 2] += (np.arange(n) // 56) % 5                                 # ... moved a few pixels along, so neighbours differ
    shift = np.ascontiguousarray(np.stack([np.arange(n) % 3 - 1, np.arange(n) % 2], axis=1).astype(np.int32))
    ref = NumpyStack(n, 1, shift)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, 1, shift)
        for off in ((1, -1), (2, -1)):
            surf, refused = layer_of(ctx, xy, off, 7, 1, shift)
            ref.add(surf, refused)
            ctx.stack_add(xy, off, 7)
        third = np.ascontiguousarray(surf[::-1])                         # a caller's layer over the same edge
        third_refused = (np.arange(n) % 7 == 0) | (np.arange(n) >= n - 2)
        ref.add(third, third_refused)
        ctx.stack_add_surfaces(third, third_refused)
        check_finish(ctx, ref, "N = STACK_CHUNK + 1", npeaks_list=(0, 2), min_counts=(1, 3))


# ---- 6. refusals ----
def test_refusals(api):
    i0, i1 = fb_pair()
    xy, shift = fb_points()
    n = xy.shape[0]

    def code(fn, *a, **k):
        with pytest.raises(api.Mimc3Error) as e:
            fn(*a, **k)
        return e.value.code

    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        surf = np.zeros((n, 81), np.float32)
        assert ctx.stack_info() == (0, 0, 0)
        assert code(ctx.stack_add, xy, FB_OFFSET, 7) == ESTATE           # an add before begin
        assert api._lib.mimc3_stack_add_surfaces(ctx._h, surf, None, n) == ESTATE
        assert code(ctx.stack_finish) == ESTATE
        assert code(ctx.stack_begin, n, 0) == EINVAL and code(ctx.stack_begin, n, 16) == EINVAL
        assert ctx.stack_info() == (0, 0, 0)
        ctx.stack_begin(n, 4, shift)
        ctx.stack_add(xy, FB_OFFSET, 7)
        before = ctx.stack_finish(3, 1, surface=True)
        assert code(ctx.stack_add, xy[:-1], FB_OFFSET, 7) == EINVAL      # a different N
        assert code(ctx.stack_add_surfaces, surf[:-1]) == EINVAL
        assert code(ctx.stack_add, xy, FB_OFFSET, 8) == EINVAL           # ocw 8
        bad = xy.copy()
        bad[3, 2] = 3.0
        assert code(ctx.stack_add, bad, FB_OFFSET, 7) == EBOUNDS         # a chip that leaves the image
        assert code(ctx.stack_add, xy, (300, 0), 7) == EBOUNDS           # a box that leaves the zero border
        assert code(ctx.stack_finish, 0, 0) == EINVAL and code(ctx.stack_finish, 0, 65536) == EINVAL      # min_count
        out, cand = np.empty((n, 8), np.float32), np.empty((8, n, 3), np.float32)
        fin = api._lib.mimc3_stack_finish
        assert fin(ctx._h, 2, 1, out, None, None, None) == EINVAL        # npeaks and cand that do not match
        assert fin(ctx._h, 0, 1, out, cand.ctypes.data, None, None) == EINVAL
        assert fin(ctx._h, 9, 1, out, cand.ctypes.data, None, None) == EINVAL
        assert ctx.stack_info() == (n, 4, 1)
        after = ctx.stack_finish(3, 1, surface=True)                     # the bytes from before the refused adds
        for a, b, what in zip(after, before, ("record", "candidates", "count", "surface")):
            assert_bits_equal(a.astype(np.float32), b.astype(np.float32), "after the refusals: " + what)
        # set_images between adds keeps the stack
        ref = NumpyStack(n, 4, shift).add(before[3], refused_of(before[0]))
        j0, j1 = fb_pair(seed=43)
        ctx.set_images(j0, j1)
        ctx.filter_images(api.CLI_KERNELS[0])
        ctx.set_images(j0, j1)
        ref.add(*layer_of(ctx, xy, FB_OFFSET, 7, 4, shift))
        ctx.stack_add(xy, FB_OFFSET, 7)
        check_finish(ctx, ref, "two pairs", npeaks_list=(3,))
        # stack_begin again resets the layers; N = 0 releases
        ctx.stack_begin(n, 4)
        assert ctx.stack_info() == (n, 4, 0)
        assert (ctx.stack_finish()[0][:, 2] == -3).all()
        ctx.stack_begin(0, 0)
        assert ctx.stack_info() == (0, 0, 0) and code(ctx.stack_finish) == ESTATE


# ---- 7. the _dev entries ----
def test_dev_entries_on_a_stream(api):
    import hipmem
    from hipmem import DevArray
    ocw, radius, npeaks = 16, 7, 3
    i0, i1, _ = class_pair("dn16")
    xy, shift = fb_points(ocw=ocw, radius=radius)
    n, NC = xy.shape[0], (2 * radius + 1) ** 2
    extra = np.random.default_rng(3).random((n, NC)).astype(np.float32)
    extra_refused = np.arange(n) % 5 == 0
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin(n, radius, shift)
        ctx.stack_add(xy, FB_OFFSET, ocw)
        ctx.stack_add_surfaces(extra, extra_refused)
        ctx.stack_add(xy, (2, -1), ocw, swap=True)
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
        ctx.stack_add_dev(d_xy.ptr, n, FB_OFFSET, ocw, stream=st.value)
        ctx.stack_add_surfaces_dev(d_extra.ptr + 4, n, d_refused=d_ref.ptr, stream=st.value)
        ctx.stack_add_dev(d_xy.ptr, n, (2, -1), ocw, stream=st.value, swap=True)
        ctx.stack_finish_dev(npeaks, 2, d_out.ptr, d_cand=d_cand.ptr, d_surf=d_surf.ptr, d_count=d_count.ptr, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.stack_info() == (n, radius, 3)
        assert_bits_equal(d_out.numpy(), want[0], "_dev: record")
        assert_bits_equal(d_cand.numpy(), want[1], "_dev: candidates")
        assert np.array_equal(d_count.numpy(), want[2])
        assert_bits_equal(d_surf.numpy(), want[3], "_dev: mean surface")
        assert hipmem._hip.hipStreamDestroy(st) == 0
