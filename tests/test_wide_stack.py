"""GPU: NCC stacking beyond +-15 px (mimc3_stack_begin_wide, stack_tail_wide_kernel in stack_kernel.hip).

Every comparison is bit for bit (NaNs by position).  A stack of one layer returns the bytes of match_ncc_wide; a stack of several layers
returns what the numpy definition (tests/stack_common.py) makes of the same layers' surfaces, which match_ncc_wide(..., surface=True)
serves; crafted surfaces at S = 95 and S = 33 exercise ties, plateaus, borders, NaN, Inf and the last cell group of the candidate
tail's bit plane; the chunk edge at mimc3_stack_chunk(R) + 1 points; R <= 15 through the new entry is the old one; refusals leave the
stack's bytes alone; the _dev entries on a stream of their own."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import float_case
from full_fb_common import FB_OFFSET, fb_pair, fb_points
from stack_common import NumpyStack, refused_of
from wide_common import FAR_OCW, far_case, fixture

pytestmark = pytest.mark.gpu

WIDE = "f32g_wide"
EINVAL, EBOUNDS = -1, -2


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_finish(ctx, ref, what, npeaks_list=(0, 3, 8), min_counts=(1,), surface=True):
    """ctx's stack against the numpy stack `ref`: record, candidates, count and (surface) the mean surface"""
    assert ctx.stack_info() == (ref.n, ref.radius, ref.layers), what
    for mc in min_counts:
        for npeaks in npeaks_list:
            got = ctx.stack_finish(npeaks, mc, surface=surface)
            w_rec, w_cand, w_lay, w_mean = ref.finish(npeaks, mc)
            tag = f"{what}: npeaks {npeaks} min_count {mc}"
            assert got[2].dtype == np.uint16 and np.array_equal(got[2], w_lay), tag + ": count"
            if surface:
                assert_bits_equal(got[3], w_mean, tag + ": mean surface")
            assert_bits_equal(got[0], w_rec, tag + ": record")
            assert (got[1] is None) == (npeaks == 0)
            if npeaks:
                assert_bits_equal(got[1], w_cand, tag + ": candidates")
    return got[0]


# ---- 1. one layer is the wide call ----
ONE_LAYER = [("u8", None, 7, 16, 0.03, False, True), ("u16", None, 7, 47, 0.03, False, True), ("u8", None, 16, 24, 0.10, False, True),
             ("u8", None, 40, 39, 0.03, False, True)]


@pytest.mark.parametrize("case", ONE_LAYER, ids=lambda c: f"ocw{c[2]}-R{c[3]}")
def test_one_layer_equals_match_ncc_wide(api, case):
    f = fixture(case)
    xy, off, ocw, R, shift = f["xy"], f["off"], f["ocw"], f["R"], f["shift"]
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add(xy, off, ocw, swap=f["swap"])
        assert ctx.last_path() == WIDE
        assert ctx.stack_info() == (n, R, 1)
        for npeaks in (0, 3, 8):
            what = f"{f['what']} npeaks {npeaks}"
            rec, cand, count, surf = ctx.stack_finish(npeaks, 1, surface=True)
            w = ctx.match_ncc_wide(xy, off, ocw, R, npeaks, shift=shift, swap=f["swap"], surface=True)
            assert_bits_equal(rec, w[0], what + ": record")
            assert_bits_equal(surf, w[2], what + ": surface")
            assert np.array_equal(count, (~refused_of(w[0])).astype(np.uint16)), what + ": count"
            if npeaks:
                assert_bits_equal(cand, w[1], what + ": candidates")
            else:
                assert cand is None
    # the fixture holds what it is for: fitted points, a status -4 point with interior candidates, a status -3 point
    assert np.isfinite(rec[:, 0]).sum() >= 5 and rec[f["g4"], 2] == -4 and rec[f["g3"], 2] == -3
    assert count[f["g3"]] == 0 and (cand[:, f["g3"], 2] == -3).all() and (cand[:, f["g4"], 2] >= -1).all()


# ---- 2. several layers against the numpy definition ----
def test_three_layers_against_numpy(api):
    R = 18
    c, f0, f1, shift = float_case(16, 0.03, R, "nan_zero")
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    n = xy.shape[0]
    f1 = f1.copy()
    # nulls in reach: the left 30 of the 51 columns of point 7's ocw-7 search box (59 % of it) -- every ocw-7 window with su <= -3 lies
    # inside them and has no pixel pair (NaN), while the wider windows of ocw 15 and the swapped layer keep some
    p = 7
    cu = int(xy[p, 2]) + int(c.offset[0]) + int(shift[p, 0])
    cv = int(xy[p, 3]) + int(c.offset[1]) + int(shift[p, 1])
    f1[cv - 25:cv + 26, cu - 25:cu + 5] = 0
    layers = ((7, False), (15, False), (16, True))
    ref = NumpyStack(n, R, shift)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        ctx.stack_begin_wide(n, R, shift)
        for ocw, swap in layers:
            rec, _, surf = ctx.match_ncc_wide(xy, c.offset, ocw, R, 0, shift=shift, swap=swap, surface=True)
            assert ctx.last_path() == WIDE
            ref.add(surf, refused_of(rec))
            ctx.stack_add(xy, c.offset, ocw, swap=swap)
        assert (ref.cnt[p] < 3).any() and (ref.cnt[p] == 3).any() and (ref.lay > 0).sum() >= 10
        rec = check_finish(ctx, ref, "ocw 7 / 15 / 16 swapped at R 18", npeaks_list=(0, 3), min_counts=(1, 3))
    assert np.isnan(ref.mean(3)[p]).any() and np.isfinite(rec[:, 0]).sum() >= 5


# ---- 3. crafted surfaces ----
NCRAFT = 7


def crafted(R, nlayers=3, seed=5):
    """Seven points -> (list of surfaces float32[7][S^2], refused bool[7]).  The crafted cells hold the same value in every layer, so
    their mean is that value exactly ((3 v) / 3 in f64); everything else is a layer's own noise in (-0.3, 0.2).
    0  nine interior maxima, a few cells apart, exactly tied at 0.75: the first by k is the record, the first eight the candidates;
    1  a plateau, a 3 x 3 block of 0.6: its lowest k alone is a local maximum -- the record and the first candidate;
    2  the best value on the border (k = S - 1 + S), lower interior peaks: -4, the interior ones are the candidates;
    3  all NaN: -2;
    4  as point 0, refused in every layer: -3;
    5  +Inf and -Inf cells, among them the centre in layer 1: they add nothing;
    6  the maximum in the last cell group that the surface reaches in the candidate tail's bit plane (word 4, k >= 64 * 32 * 4, at
       S = 95; word 0's last bit, k >= 1024, at S = 33)."""
    S = 2 * R + 1
    NC = S * S
    rng = np.random.default_rng(seed + R)
    ctr = R * S + R
    ties = [(3 + 4 * i) * S + (4 + 3 * j) for i in range(3) for j in range(3)]
    last = (S - 5) * S + R if S == 95 else (S - 2) * S + 10
    assert last >= (64 * 32 * 4 if S == 95 else 1024) and last < NC - S
    layers = []
    for k in range(nlayers):
        s = (rng.random((NCRAFT, NC)) * 0.5 - 0.3).astype(np.float32)
        s[0, ties] = 0.75
        s[4] = s[0]
        for x in (20, 21, 22):
            s[1, x * S + 8:x * S + 11] = 0.6
        s[2, ctr] = 0.5
        s[2, ctr + 5 * S + 3] = 0.4
        s[2, 2 * S - 1] = 0.9
        s[3] = np.nan
        s[5, ctr] = 0.8 if k != 1 else np.inf
        inf_cells = rng.choice(NC, 4, replace=False)
        s[5, inf_cells[:2]] = np.inf
        s[5, inf_cells[2:]] = -np.inf
        s[6, last] = 0.7
        layers.append(np.ascontiguousarray(s))
    refused = np.zeros(NCRAFT, bool)
    refused[4] = True
    return layers, refused, ties, last


@pytest.mark.parametrize("radius", (47, 16))
def test_crafted_surfaces(api, radius):
    layers, refused, ties, last = crafted(radius)
    S = 2 * radius + 1
    ref = NumpyStack(NCRAFT, radius)
    with api.Context(0) as ctx:                                          # (no images: add_surfaces needs none)
        ctx.stack_begin_wide(NCRAFT, radius)
        check_finish(ctx, ref, f"R {radius}: an empty stack", npeaks_list=(0, 3))
        for s in layers:
            ref.add(s, refused)
            ctx.stack_add_surfaces(s, refused)
        check_finish(ctx, ref, f"R {radius}: three layers", min_counts=(1, 3))
        rec, cand, count, mean = ctx.stack_finish(8, 1, surface=True)
    assert count.tolist() == [3, 3, 3, 3, 0, 3, 3]
    # the ties: the record is the first by k, the candidates the first eight in k order
    assert rec[0, 2] == np.float32(0.75) and (cand[:, 0, 2] == np.float32(0.75)).all()
    want = [(k // S - radius, k % S - radius) for k in sorted(ties)]
    assert (np.rint(rec[0, :2]) == want[0]).all()
    assert [tuple(np.rint(cand[j, 0, :2]).astype(int)) for j in range(8)] == want[:8]
    # the plateau: one local maximum, not nine
    assert rec[1, 2] == np.float32(0.6) and cand[0, 1, 2] == np.float32(0.6) and -1 <= cand[1, 1, 2] < np.float32(0.5)
    assert rec[2, 2] == -4 and cand[0, 2, 2] == np.float32(0.5) and cand[1, 2, 2] == np.float32(0.4)
    assert rec[3, 2] == -2 and (cand[:, 3, 2] == -2).all()
    assert rec[4, 2] == -3 and (cand[:, 4, 2] == -3).all()
    assert rec[5, 2] == np.float32(0.8) and np.isfinite(mean[5]).all()   # Inf cells: no trace in the mean
    assert rec[6, 2] == np.float32(0.7) and cand[0, 6, 2] == np.float32(0.7)
    assert (np.rint(rec[6, :2]) == (last // S - radius, last % S - radius)).all()


# ---- 4. the chunk edge ----
def test_chunk_edge_of_a_searched_layer(api):
    """N = stack_chunk(16) + 1 at ocw 7: the second launch of the search and of the accumulation holds one point"""
    R, ocw = 16, 7
    n = api.stack_chunk(R) + 1
    i0, i1 = fb_pair()
    base, _ = fb_points(ocw=ocw, radius=R)
    xy = np.ascontiguousarray(base[np.arange(n) % 56])                   # the grid's 56 points over and over, plus one
    xy[:, 2] += (np.arange(n) // 56) % 5                                 # ... moved a few pixels along, so neighbours differ
    shift = np.ascontiguousarray(np.stack([np.arange(n) % 3 - 1, np.arange(n) % 2], axis=1).astype(np.int32))
    xy[-1], shift[-1] = base[9], (1, 0)                                  # the point beyond the edge: one whose true peak is interior
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add(xy, FB_OFFSET, ocw)
        assert ctx.last_path() == WIDE
        rec, cand, count = ctx.stack_finish(2, 1)
        w_rec, w_cand = ctx.match_ncc_wide(xy, FB_OFFSET, ocw, R, 2, shift=shift)
    assert_bits_equal(rec, w_rec, "N = stack_chunk(16) + 1: record")
    assert_bits_equal(cand, w_cand, "N = stack_chunk(16) + 1: candidates")
    assert np.array_equal(count, (~refused_of(w_rec)).astype(np.uint16))
    assert np.isfinite(rec[-1, 0]) and np.isfinite(rec[:, 0]).mean() > 0.2


def test_chunk_edge_of_a_callers_layer(api):
    """N = stack_chunk(47) + 1 surfaces of 95 x 95 cells: a tiling of the crafted ones"""
    R = 47
    n = api.stack_chunk(R) + 1
    layers, refused, _, _ = crafted(R, nlayers=1)
    ref = NumpyStack(NCRAFT, R).add(layers[0], refused)
    idx = np.arange(n) % NCRAFT
    with api.Context(0) as ctx:
        ctx.stack_begin_wide(n, R)
        ctx.stack_add_surfaces(layers[0][idx], refused[idx])
        rec, cand, count = ctx.stack_finish(2, 1)
    w_rec, w_cand, w_lay, _ = ref.finish(2, 1)
    assert_bits_equal(rec, w_rec[idx], "N = stack_chunk(47) + 1: record")
    assert_bits_equal(cand, w_cand[:, idx], "N = stack_chunk(47) + 1: candidates")
    assert np.array_equal(count, w_lay[idx])


# ---- 5. R <= 15 through the new entry is the old one ----
@pytest.mark.parametrize("radius", (4, 15))
def test_begin_wide_at_small_radius_is_stack_begin(api, radius):
    i0, i1 = fb_pair()
    xy, shift = fb_points(ocw=16, radius=radius)                         # (every chip inside the image at both chip sizes)
    n = xy.shape[0]
    extra = np.random.default_rng(radius).random((n, (2 * radius + 1) ** 2)).astype(np.float32)
    got = []
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for begin in (ctx.stack_begin, ctx.stack_begin_wide):
            begin(n, radius, shift)
            ctx.stack_add(xy, FB_OFFSET, 7)
            assert ctx.last_path() == "f32g_full"
            ctx.stack_add_surfaces(extra, np.arange(n) % 4 == 0)
            ctx.stack_add(xy, (2, -1), 16, swap=True)
            assert ctx.stack_info() == (n, radius, 3)
            got.append([ctx.stack_finish(k, mc, surface=True) for k in (0, 3) for mc in (1, 2)])
    for a, b in zip(*got):
        for x, y, what in zip(a, b, ("record", "candidates", "count", "surface")):
            if x is None:
                assert y is None
            else:
                assert x.tobytes() == y.tobytes(), f"R {radius}: {what}"


# ---- 6. refusals ----
def test_refusals(api):
    c = far_case()
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    n = xy.shape[0]

    def code(fn, *a, **k):
        with pytest.raises(api.Mimc3Error) as e:
            fn(*a, **k)
        return e.value.code

    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        assert code(ctx.stack_begin_wide, n, 0) == EINVAL and code(ctx.stack_begin_wide, n, 48) == EINVAL
        assert code(ctx.stack_begin, n, 16) == EINVAL                    # the old entry keeps its range
        assert ctx.stack_info() == (0, 0, 0)
        ctx.stack_begin_wide(n, 40)
        ctx.stack_add(xy, (0, 0), FAR_OCW)
        before = ctx.stack_finish(3, 1, surface=True)
        assert api.wide_max_radius(40) < 40
        assert code(ctx.stack_add, xy, (0, 0), 40) == EINVAL             # ocw 40 does not reach R 40
        assert code(ctx.stack_add, xy, (0, 0), 8) == EINVAL              # ocw 8
        assert code(ctx.stack_add, xy[:-1], (0, 0), FAR_OCW) == EINVAL   # a different N
        assert code(ctx.stack_add_surfaces, np.zeros((n - 1, 81 * 81), np.float32)) == EINVAL
        assert code(ctx.stack_add, xy, (300, 0), FAR_OCW) == EBOUNDS     # a box that leaves the zero border
        assert ctx.stack_info() == (n, 40, 1)
        after = ctx.stack_finish(3, 1, surface=True)
        for a, b, what in zip(after, before, ("record", "candidates", "count", "surface")):
            assert a.tobytes() == b.tobytes(), "after the refusals: " + what
        assert np.isfinite(before[0][:, 0]).all()
        ctx.stack_begin_wide(0, 0)
        assert ctx.stack_info() == (0, 0, 0)


# ---- 7. the _dev entries ----
def test_dev_entries_on_a_stream(api):
    import hipmem
    from hipmem import DevArray
    R, ocw, npeaks = 20, 16, 3
    c, f0, f1, shift = float_case(ocw, 0.03, R, "nan_zero")
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    n, NC = xy.shape[0], (2 * R + 1) ** 2
    extra = np.random.default_rng(3).random((n, NC)).astype(np.float32)
    extra_refused = np.arange(n) % 5 == 0
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add(xy, c.offset, ocw)
        ctx.stack_add_surfaces(extra, extra_refused)
        ctx.stack_add(xy, (2, -1), 7, swap=True)
        want = ctx.stack_finish(npeaks, 2, surface=True)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        d_xy = DevArray(src=xy)
        # an unaligned caller's array: the surfaces start 4 bytes into the allocation
        d_extra = DevArray(src=np.concatenate([np.zeros(1, np.float32), extra.ravel()]))
        d_ref = DevArray(src=extra_refused.astype(np.uint8))
        d_out, d_cand = DevArray((n, 8), np.float32), DevArray((npeaks, n, 3), np.float32)
        d_surf, d_count = DevArray((n, NC), np.float32), DevArray((n,), np.uint16)
        ctx.stack_begin_wide(n, R, shift)
        ctx.stack_add_dev(d_xy.ptr, n, c.offset, ocw, stream=st.value)
        ctx.stack_add_surfaces_dev(d_extra.ptr + 4, n, d_refused=d_ref.ptr, stream=st.value)
        ctx.stack_add_dev(d_xy.ptr, n, (2, -1), 7, stream=st.value, swap=True)
        ctx.stack_finish_dev(npeaks, 2, d_out.ptr, d_cand=d_cand.ptr, d_surf=d_surf.ptr, d_count=d_count.ptr, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.stack_info() == (n, R, 3) and ctx.last_path() == WIDE
        assert_bits_equal(d_out.numpy(), want[0], "_dev: record")
        assert_bits_equal(d_cand.numpy(), want[1], "_dev: candidates")
        assert np.array_equal(d_count.numpy(), want[2])
        assert_bits_equal(d_surf.numpy(), want[3], "_dev: mean surface")
        assert hipmem._hip.hipStreamDestroy(st) == 0
    assert np.isfinite(want[0][:, 0]).sum() >= 5
