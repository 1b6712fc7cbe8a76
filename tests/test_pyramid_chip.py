"""GPU: the coarse-to-fine exhaustive search at any chip size (mimc3_match_ncc_pyramid_chip: the levels of the pair's class, one
run-time-ocw kernel on every level -- its PEAK form on the coarser ones -- the chaining on the device) against the test-side definitions
(tests/pyramid_dn_oracle.py, tests/pyramid_any_oracle.py) and against the entries it must agree with.

Every comparison is bit for bit, with two exceptions that come from the references, not from the code under test: the SNR column
against pyramid_search_dn is within 1 f32 ulp (the oracle adds its f64 sum of squares in another order; assert_records_match, as in
tests/test_pyramid_dn.py) -- the same records are compared bit for bit, SNR included, with the single-level entry at shift_out -- and
against the reference-order float oracle only the points whose coarser-level arg-max the definition determines are compared
(tests/pyramid_any_oracle.py; at most UNDECIDED_CAP of them are not).  last_path() is asserted after every call."""
import numpy as np
import pytest

import pyramid_chip_common as pc
from conftest import assert_bits_equal
from pyramid_any_oracle import UNDECIDED_CAP, pyramid_any, pyramid_search_any
from pyramid_dn_oracle import as_class, case, pyramid_search_dn, surface_peaks
from pyramid_oracle import _inside

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def path(cls, ocw, mode=0):
    return pc.PATH_NAME[pc.table_path(cls, ocw, mode)]


def same(got, want, what):
    """(record, candidates, shift_out) of two device calls: bit for bit"""
    np.testing.assert_array_equal(got[2], want[2], what + ": shift_out")
    assert_bits_equal(got[0], want[0], what + ": record")
    if want[1] is None:
        assert got[1] is None
    else:
        assert_bits_equal(got[1], want[1], what + ": candidates")


# ---- 1. oracle parity on the integer classes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,ocw", [(k, o) for k in pc.CLASSES for o in pc.PARITY_OCW] + [("u8", 80), ("u16", 80)])
def test_oracle_parity(api, cls, ocw):
    """Record, candidates and shift_out against pyramid_search_dn: ocw on both sides of the KCW thresholds, L 2 and 3, null fractions 0 and
    0.15, npeaks 0 and 4, both directions (pc.PARITY_COMBOS, the full product); ocw 80 once at R 15 on the two matrix-core classes."""
    with api.Context(0) as ctx:
        for idx, (what, c, i0, i1, off, sh_in, o, r, levels, npeaks, swap) in enumerate(pc.parity_calls(cls, ocw)):
            ctx.set_images(i0, i1)
            got = ctx.match_ncc_pyramid_chip(c.xyuvav, off, o, r, levels, npeaks, shift=sh_in, swap=swap)
            assert ctx.last_path() == path(cls, o)
            want = pc.expected(cls, ocw, idx)
            pc.compare(got, want[:3], what)
            assert (got[0][:, 2] >= -1).any() and (got[2] != sh_in).any(), what + ": nothing found"


# ---- 2. at the six ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocw", [7, 16, 40])
@pytest.mark.parametrize("cls", pc.CLASSES)
def test_at_the_six_both_modes_are_match_ncc_pyramid_dn(api, cls, ocw):
    c = case(ocw, 0.03, 9850 + ocw, 3)
    i0, i1 = (c.i0, c.i1) if cls == "u8" else as_class(cls, c, ocw)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks, swap in ((0, True), (4, False)):
            off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
            want = ctx.match_ncc_pyramid_dn(c.xyuvav, off, ocw, pc.R, 3, npeaks, shift=sh_in, swap=swap)
            assert ctx.last_path() == {"u8": "u8_mfma_full", "u16": "u16_full", "f32": "f32i_full"}[cls]
            for mode in (0, 1):
                got = ctx.match_ncc_pyramid_chip(c.xyuvav, off, ocw, pc.R, 3, npeaks, shift=sh_in, swap=swap, mode=mode)
                assert ctx.last_path() == path(cls, ocw, mode)
                same(got, want, f"{cls} ocw {ocw} mode {mode} npeaks {npeaks} swap {swap}")
        assert (want[0][:, 2] >= -1).any() and (want[2] != sh_in).any()


@pytest.mark.parametrize("ocw", [7, 16, 40])
def test_at_the_six_mode0_on_a_float_pair_is_match_ncc_pyramid_any(api, ocw):
    c, f0, f1, shift = pc.float_case(ocw, 0.03, 3)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        want = ctx.match_ncc_pyramid_any(c.xyuvav, c.offset, ocw, pc.R, 3, 4, shift=shift)
        assert ctx.last_path() == "f32g_full"
        got = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, ocw, pc.R, 3, 4, shift=shift)
        assert ctx.last_path() == path("float", ocw) == "f32g_full"
        same(got, want, f"float ocw {ocw}")


# ---- 3. level 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocw", [10, 45, 57])
@pytest.mark.parametrize("cls", pc.CLASSES)
def test_level0_is_the_single_level_entry_at_shift_out(api, cls, ocw):
    """Record and candidates equal match_ncc_full_chip_planes(mode 0, shift = shift_out), all eight columns bit for bit."""
    with api.Context(0) as ctx:
        for idx, (what, c, i0, i1, off, sh_in, o, r, levels, npeaks, swap) in pc.pick(cls, ocw, 3, 4) + pc.pick(cls, ocw, 2, 0)[:1]:
            ctx.set_images(i0, i1)
            rec, cand, sh = ctx.match_ncc_pyramid_chip(c.xyuvav, off, o, r, levels, npeaks, shift=sh_in, swap=swap)
            assert ctx.last_path() == path(cls, o)
            full = ctx.match_ncc_full_chip_planes(c.xyuvav, off, o, r, npeaks, shift=sh, swap=swap)      # (accepted: every box inside the border)
            assert ctx.last_path() == path(cls, o)
            assert_bits_equal(rec, full[0], what + ": record vs the single-level entry")
            if npeaks:
                assert_bits_equal(cand, full[1], what + ": candidates vs the single-level entry")


@pytest.mark.parametrize("cls", pc.CLASSES + ("float",))
def test_level_borders_are_zero(api, cls):
    """check_border of tests/test_pyramid_dn.py at a chip size outside the six: every point's level-1 box starts on the first border column
    right of the level image and the level-0 box lies in the border too -- no arg-max on level 1 (d_0 = 2 d_1), status -3 on level 0."""
    ocw, h = 10, 10 + 1
    if cls == "float":
        c, i0, i1, _ = pc.float_case(10, 0.03, 2)
    else:
        c, i0, i1, _ = pc.pair(cls, 10, 0.15, 2)
    W = i0.shape[1]
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    u0 = xy[:, 2].astype(np.int64)
    d1 = (W >> 1) + h - (u0 >> 1)
    shift = np.stack([2 * d1, np.zeros_like(d1)], axis=1).astype(np.int32)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.match_ncc_pyramid_chip(xy, (0, 0), ocw, 1, 2)                  # (peaks in the scratch first)
        rec, _, sh = ctx.match_ncc_pyramid_chip(xy, (0, 0), ocw, 1, 2, shift=shift)
        assert ctx.last_path() == path(cls, ocw)
    np.testing.assert_array_equal(sh, shift, cls + ": level 1 found an arg-max in the border")
    assert (rec[:, 2] == -3).all(), cls + f": statuses {rec[:, 2].tolist()}"


# ---- 4. the float class -------------------------------------------------------------------------------------------------------------
def chain(api, f0, f1, xyuvav, offset, ocw, radius, levels, shift, swap):
    """shift_out as a caller gets it by chaining match_ncc_full_chip(mode 1, surface) over the numpy-built float levels by hand (the chain
    of tests/test_pyramid_any.py with that entry)."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    off = np.asarray(offset, np.int64).reshape(1, 2)
    D = off + (np.zeros((n, 2), np.int64) if shift is None else np.asarray(shift, np.int64))
    uv0 = xy[:, 2:4].astype(np.int64)
    d = D if levels == 1 else (D + (1 << (levels - 2))) >> (levels - 1)
    p0, p1 = pyramid_any(f0, levels), pyramid_any(f1, levels)
    S = 2 * radius + 1
    for lv in range(levels - 1, 0, -1):
        H, W = p0[lv].shape
        pos = uv0 >> lv
        ok = _inside(pos, d, ocw, radius, H, W)
        pk = np.full(n, -1, np.int64)
        if ok.any():
            lxy = np.zeros((int(ok.sum()), 6))
            lxy[:, 2:4] = pos[ok]
            with api.Context(0) as lctx:
                lctx.set_images(p0[lv], p1[lv])
                surf = lctx.match_ncc_full_chip(lxy, (0, 0), ocw, radius, 0, shift=d[ok].astype(np.int32), swap=swap, mode=1, surface=True)[2]
                assert lctx.last_path() == "f32g_chip"
            pk[ok] = surface_peaks(surf)
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - radius, pk % S - radius], axis=1), 0)
        d = 2 * (d + s)
    return (d - off).astype(np.int32)


@pytest.mark.parametrize("levels,swap,null_frac", [(2, False, 0.03), (3, True, 0.0)])
@pytest.mark.parametrize("ocw", pc.FLOAT_OCW)
def test_float_class_is_the_chain_of_single_level_calls(api, ocw, levels, swap, null_frac):
    c, f0, f1, shift = pc.float_case(ocw, null_frac, levels)
    off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
    what = f"float ocw {ocw} nulls {null_frac} L {levels} swap {swap}"
    want_sh = chain(api, f0, f1, c.xyuvav, off, ocw, pc.R, levels, sh_in, swap)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for npeaks in (0, 4):
            rec, cand, sh = ctx.match_ncc_pyramid_chip(c.xyuvav, off, ocw, pc.R, levels, npeaks, shift=sh_in, swap=swap)
            assert ctx.last_path() == path("float", ocw) == "f32g_chip"
            np.testing.assert_array_equal(sh, want_sh, what)
            full = ctx.match_ncc_full_chip(c.xyuvav, off, ocw, pc.R, npeaks, shift=sh, swap=swap, mode=1)
            assert_bits_equal(rec, full[0], what + f": record vs match_ncc_full_chip, npeaks {npeaks}")
            if npeaks:
                assert_bits_equal(cand, full[1], what + ": candidates vs match_ncc_full_chip")
            else:
                assert cand is None
            m1 = ctx.match_ncc_pyramid_chip(c.xyuvav, off, ocw, pc.R, levels, npeaks, shift=sh_in, swap=swap, mode=1)
            assert ctx.last_path() == "f32g_chip"
            same(m1, (rec, cand, sh), what + ": mode 1")
        assert (rec[:, 2] >= -1).any() and (sh != sh_in).any()


def test_float_class_against_the_reference_order_oracle(api):
    c, f0, f1, shift, ocw, r, levels = pc.float_oracle_case()
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        rec, _, sh = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, ocw, r, levels, shift=shift)
        assert ctx.last_path() == "f32g_chip"
    want, _, want_sh, und = pyramid_search_any(f0, f1, c.xyuvav, c.offset, ocw, r, levels, shift=shift)
    print(f"{int(und.sum())} of {c.n} points undecided")
    assert und.mean() <= UNDECIDED_CAP
    np.testing.assert_array_equal(sh[~und], want_sh[~und])
    np.testing.assert_array_equal(rec[~und, 2] == -3, want[~und, 2] == -3)
    assert (rec[~und, 2] >= -1).any()


# ---- 5. stale peaks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", pc.CLASSES + ("float",))
def test_a_point_without_an_arg_max_does_not_keep_the_last_calls_peak(api, cls):
    """One context, two calls: the first leaves a peak at every index; the second has, at four of the same indices, no arg-max on level 1
    (the chip leaves the level, the box lies beyond the border, -3, -2: pc.stale_case; tests/test_pyramid_chip_cpu.py checks the reasons).
    A missed peak store would step from the first call's cell."""
    s = pc.STALE
    i0, i1, xy1, xy2, shift2 = pc.stale_case(cls)
    idx = sorted(pc.STALE_POINTS)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        first = ctx.match_ncc_pyramid_chip(xy1, (0, 0), s["ocw"], s["R"], s["levels"], 2)
        assert ctx.last_path() == path(cls, s["ocw"])
        second = ctx.match_ncc_pyramid_chip(xy2, (0, 0), s["ocw"], s["R"], s["levels"], 2, shift=shift2)
        assert ctx.last_path() == path(cls, s["ocw"])
    if cls == "float":
        w1 = pyramid_search_any(i0, i1, xy1, (0, 0), s["ocw"], s["R"], s["levels"], 2)
        w2 = pyramid_search_any(i0, i1, xy2, (0, 0), s["ocw"], s["R"], s["levels"], 2, shift=shift2)
        assert not w2[3][idx].any() and w1[3].mean() <= UNDECIDED_CAP and w2[3].mean() <= UNDECIDED_CAP
        for got, want in ((first, w1), (second, w2)):
            ok = ~want[3]
            np.testing.assert_array_equal(got[2][ok], want[2][ok])
            np.testing.assert_array_equal(np.isnan(got[0][ok, 2]), np.isnan(want[0][ok, 2]))
            np.testing.assert_array_equal(got[0][ok, 2] == -3, want[0][ok, 2] == -3)
    else:
        w1 = pyramid_search_dn(i0, i1, xy1, (0, 0), s["ocw"], s["R"], s["levels"], 2)
        w2 = pyramid_search_dn(i0, i1, xy2, (0, 0), s["ocw"], s["R"], s["levels"], 2, shift=shift2)
        pc.compare(first, w1, cls + ": first call")
        pc.compare(second, w2, cls + ": second call")
    assert first[2][idx].any(axis=1).all()                              # the first call's peaks there were not the centre cell
    np.testing.assert_array_equal(second[2][idx], shift2[idx])          # no arg-max on level 1: d_0 = 2 d_1
    assert np.isnan(second[0][1]).all() and second[0][2, 2] == -3 and second[0][3, 2] == -2


# ---- 6. a filtered pair, and a new pair ---------------------------------------------------------------------------------------------------
def class_of(f0, f1):
    """The class the library gives an integer pair (tests/test_pyramid_dn.py)"""
    if all((f == np.rint(f)).all() and f.max() <= 255 for f in (f0, f1)):
        return "u8"
    q = [f if (f == np.rint(f)).all() else f * np.float32(8) for f in (f0, f1)]
    return "u16" if all(v.max() < 4096 for v in q) else "f32"


def test_filtered_8bit_pair_then_a_new_pair(api):
    """Filter, then reduce: the oracle reads the filtered planes as ctx.get_images() returns them.  Then set_images: the levels follow."""
    c, i0, i1, shift = pc.pair("u8", 10, 0.15, 2)
    b, j0, j1, bshift = pc.pair("u16", 10, 0.0, 2)
    H, W = i0.shape
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        raw = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, 10, pc.R, 2, 4, shift=shift)      # (the raw pair's levels are built ...)
        assert ctx.last_path() == "u8_mfma_chip"
        ctx.filter_images(api.CLI_KERNELS[1])                                                   # (... and must not outlive the filter)
        f0, f1 = ctx.get_images(H, W)
        cls = class_of(f0, f1)
        got = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, 10, pc.R, 2, 4, shift=shift)
        assert ctx.last_path() == path(cls, 10)
        pc.compare(got, pyramid_search_dn(f0, f1, c.xyuvav, c.offset, 10, pc.R, 2, 4, shift=shift), "filtered 8-bit pair (" + cls + ")")
        assert not np.array_equal(got[2], raw[2]) or not np.array_equal(got[0], raw[0], equal_nan=True)
        ctx.filter_images(None)
        same(ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, 10, pc.R, 2, 4, shift=shift), raw, "unfiltered again")
        ctx.set_images(j0, j1)
        got = ctx.match_ncc_pyramid_chip(b.xyuvav, b.offset, 10, pc.R, 2, 4, shift=bshift)
        assert ctx.last_path() == "u16_mfma_chip"
        pc.compare(got, pyramid_search_dn(j0, j1, b.xyuvav, b.offset, 10, pc.R, 2, 4, shift=bshift), "a new pair")


# ---- 7. the _dev twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["u8", "u16", "float"])
def test_device_twin_on_a_callers_stream(api, cls):
    import ctypes as C
    import hipmem
    from hipmem import DevArray
    if cls == "float":
        c, i0, i1, shift = pc.float_case(10, 0.03, 3)
    else:
        c, i0, i1, shift = pc.pair(cls, 25, 0.15, 3)
    ocw = c.ocw
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
        d_out, d_cand, d_sho = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32), DevArray((c.n, 2), np.int32)
        st = C.c_void_p()                                       # a caller's stream, of the runtime the library runs on
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        # (the first call on the pair: the _dev entry builds the planes and the levels itself)
        ctx.match_ncc_pyramid_chip_dev(d_xy.ptr, c.n, c.offset, ocw, pc.R, 3, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, d_shift_out=d_sho.ptr,
                                       stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == path(cls, ocw)
        dev, dev_cand, dev_sh = d_out.numpy(), d_cand.numpy(), d_sho.numpy()
        d_out2 = DevArray((c.n, 8), np.float32)
        ctx.match_ncc_pyramid_chip_dev(d_xy.ptr, c.n, c.offset, ocw, pc.R, 3, 0, d_out2.ptr, d_shift=d_sh.ptr, stream=st.value, mode=1)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == path(cls, ocw, 1)
        dev2 = d_out2.numpy()
        rec, cand, sh = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, ocw, pc.R, 3, 4, shift=shift)
        rec0 = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, ocw, pc.R, 3, 0, shift=shift, mode=1)[0]
        assert hipmem._hip.hipStreamDestroy(st) == 0
    assert_bits_equal(dev, rec, "_dev twin")
    assert_bits_equal(dev_cand, cand, "_dev twin: candidates")
    assert_bits_equal(dev2, rec0, "_dev twin without shift_out and candidates")
    np.testing.assert_array_equal(dev_sh, sh)
    assert (rec[:, 2] >= -1).any()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(api):
    c, i0, i1, shift = pc.pair("u16", 10, 0.0, 2)                   # 87 x 101: levels 1 and 2 hold a 21-px chip, level 3 does not
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    n = c.n
    off = np.zeros(2, np.int32)
    far = np.array([1 << 25, 0], np.int32)
    bad = xy.copy()
    bad[3, 2] = 3.0                                                 # the level-0 chip leaves the image
    call = api._lib.mimc3_match_ncc_pyramid_chip
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        #        xy, offset, ocw, R, levels, npeaks, mode, cand given, code
        cases = [(xy, off, 10, pc.R, 0, 0, 0, False, -1), (xy, off, 10, pc.R, 6, 0, 0, False, -1),
                 (xy, off, 0, pc.R, 2, 0, 0, False, -1), (xy, off, 81, pc.R, 2, 0, 0, False, -1),
                 (xy, off, 10, 0, 2, 0, 0, False, -1), (xy, off, 10, 16, 2, 0, 0, False, -1),
                 (xy, off, 10, pc.R, 2, 9, 0, True, -1),
                 (xy, off, 10, pc.R, 2, 2, 0, False, -1), (xy, off, 10, pc.R, 2, 0, 0, True, -1),
                 (xy, off, 10, pc.R, 2, 0, 2, False, -1), (xy, off, 10, pc.R, 2, 0, -1, False, -1),
                 (xy, off, 10, pc.R, 4, 0, 0, False, -1),           # level 3 is 10 x 12: smaller than the chip
                 (xy, far, 10, pc.R, 2, 0, 0, False, -1),
                 (bad, off, 10, pc.R, 2, 0, 0, False, -2)]
        for k, (pts, o, ocw, r, levels, npeaks, mode, with_cand, code) in enumerate(cases):
            out = np.full((n, 8), 7.5, np.float32)
            cand = np.full((9, n, 3), 7.5, np.float32)
            sho = np.full((n, 2), 77, np.int32)
            rc = call(ctx._h, pts, n, o, None, ocw, r, levels, npeaks, 0, mode, out, cand.ctypes.data if with_cand else None, sho)
            assert rc == code, f"case {k}: rc {rc}"
            assert (out == 7.5).all() and (cand == 7.5).all() and (sho == 77).all(), f"case {k}: an output buffer was written"
        assert min(i0.shape) >> 2 >= 21 > min(i0.shape) >> 3
        got = ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, 10, pc.R, 2, shift=shift)      # the context still works
        assert ctx.last_path() == "u16_mfma_chip"
        pc.compare(got, pyramid_search_dn(i0, i1, c.xyuvav, c.offset, 10, pc.R, 2, shift=shift), "after the refusals")
    with api.Context(0) as ctx:                                     # no images: MIMC3_ESTATE
        out = np.full((n, 8), 7.5, np.float32)
        sho = np.full((n, 2), 77, np.int32)
        assert call(ctx._h, xy, n, off, None, 10, pc.R, 2, 0, 0, 0, out, None, sho) == -5
        assert (out == 7.5).all() and (sho == 77).all()


# ---- 9. candidates over variants ------------------------------------------------------------------------------------------------------
def test_full_candidates_over_levels(api):
    c = case(16, 0.03, 9871, 2)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    kernels = (None, api.CLI_KERNELS[2])
    vec_ocw = (10, 16)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        dp = ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, pc.R, 2, kernels=kernels, shift=shift, levels=2)
        before = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, pc.R, 2, shift=shift)        # the pair is left unfiltered
        blocks, paths = [], []
        for k in kernels:
            ctx.filter_images(None)
            if k is not None:
                ctx.filter_images(k)
            for ocw in vec_ocw:
                blocks.append(ctx.match_ncc_pyramid_chip(c.xyuvav, c.offset, ocw, pc.R, 2, 2, shift=shift)[1])
                paths.append(ctx.last_path())
        ctx.filter_images(None)
        assert paths == ["u8_mfma_chip", "u8_mfma_full", "u16_mfma_chip", "u16_mfma_chip"]
        assert dp.shape == (8, c.n, 3)
        assert_bits_equal(dp, np.concatenate(blocks, axis=0), "levels = 2")
        assert_bits_equal(before[0], ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, pc.R, 2, shift=shift)[0], "the pair after full_candidates")
        # levels = 1: exactly the calls of today
        one = ctx.full_candidates(c.xyuvav, c.offset, (16, 7), pc.R, 2, kernels=kernels, shift=shift, levels=1)
        assert_bits_equal(one, ctx.full_candidates(c.xyuvav, c.offset, (16, 7), pc.R, 2, kernels=kernels, shift=shift), "levels = 1 vs the default")
        blocks = []
        for k in kernels:
            ctx.filter_images(None)
            if k is not None:
                ctx.filter_images(k)
            for ocw in (16, 7):
                blocks.append(ctx.match_ncc_full_dn(c.xyuvav, c.offset, ocw, pc.R, 2, shift=shift)[1])
        ctx.filter_images(None)
        assert_bits_equal(one, np.concatenate(blocks, axis=0), "levels = 1")
