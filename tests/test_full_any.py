"""GPU: the exhaustive search on any f32 pair (mimc3_match_ncc_full_any, match_full_f32g_kernel.hip).

Exact where exactness exists: on 8-bit, 12-bit and 16-bit pairs the float kernel (mode 1) must return the bytes of match_ncc_full_dn and
the oracle's surface bit for bit.  On float pairs the order of the f64 additions is the kernel's own: the surface's finite mask equals
the oracle's and every finite cell is within 1 f32 ulp of it (the bound of include/mimc3_hip.h; tests/test_full_any_cpu.py shows that
the fixtures satisfy it with the reference arithmetic alone), and record and candidates are the oracle's tail of the DEVICE surface,
bit for bit -- the SNR too: tail_from_surface adds its squares in the device tail's order.  The prescribed float fixtures have exact
f64 sums in any order (their terms span 2^17), so the tolerance is only exercised on the wide-range pair (test_wide_range_pair)."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import (APART_INF, APART_OCW, APART_R, ENCODINGS, FILTERED_KERNELS, FILTERED_OCW, FILTERED_R, float_case, full_any,
                             rules_apart_case, surface_distance, tail_from_surface, to_float, wide_case)
from full_dn_common import dn16_case, periodic_pair16, status_case16
from full_multi_common import STATUS_R, parity_case
from full_planes_common import PLANES_OCW, PLANES_R, dn12_case
from full_search_common import assert_records_match
from mimc3_amd import synth

pytestmark = pytest.mark.gpu

NPEAKS = (1, 4, 8)
G = "f32g_full"


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


# ---- 1. exact where exactness exists ----
def check_exact(ctx, i0, i1, xy, off, ocw, radius, shift, swap, what):
    """mode 1 on an integer-class pair: the bytes of match_ncc_full_dn, the oracle's surface."""
    want_surf = full_any(i0, i1, xy, off, ocw, radius, 0, shift=shift, swap=swap)[2]
    ref_rec, _ = ctx.match_ncc_full_dn(xy, off, ocw, radius, 0, shift=shift, swap=swap)
    assert ctx.last_path() != G
    rec, none, surf = ctx.match_ncc_full_any(xy, off, ocw, radius, 0, shift=shift, swap=swap, mode=1, surface=True)
    assert none is None and ctx.last_path() == G
    assert_bits_equal(surf, want_surf, what + ": surface vs the oracle")
    assert_records_match(rec, ref_rec, what + ": record vs match_ncc_full_dn")
    for npeaks in NPEAKS:
        ref_out, ref_cand = ctx.match_ncc_full_dn(xy, off, ocw, radius, npeaks, shift=shift, swap=swap)
        out, cand = ctx.match_ncc_full_any(xy, off, ocw, radius, npeaks, shift=shift, swap=swap, mode=1)
        assert ctx.last_path() == G and cand.shape == (npeaks, xy.shape[0], 3)
        assert_bits_equal(out, rec, what + f": record at npeaks {npeaks} vs npeaks 0")
        assert_bits_equal(cand, ref_cand, what + f": candidates vs match_ncc_full_dn, npeaks {npeaks}")


def integer_pair(bits, ocw, null_frac, radius):
    if bits == 8:
        c, shift = parity_case(ocw, null_frac, radius, dimx=5, dimy=4)
        return c, c.i0, c.i1, shift
    return (dn12_case if bits == 12 else dn16_case)(ocw, null_frac, radius)


@pytest.mark.parametrize("radius", PLANES_R)
@pytest.mark.parametrize("null_frac", [0.0, 0.03])
@pytest.mark.parametrize("ocw", PLANES_OCW)
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_mode1_equals_full_dn_on_integer_pairs(api, bits, ocw, null_frac, radius):
    c, i0, i1, shift = integer_pair(bits, ocw, null_frac, radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            check_exact(ctx, i0, i1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap,
                        f"{bits}-bit ocw {ocw} nulls {null_frac} R {radius} swap {swap}")


def test_mode1_statuses_and_ties(api):
    i0, i1, xy = status_case16()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        st = ctx.match_ncc_full_dn(xy, (0, 0), 7, STATUS_R, 0)[0][:, 2]
        assert (st == -2).any() and (st == -3).any() and (st == -4).any()
        check_exact(ctx, i0, i1, xy, (0, 0), 7, STATUS_R, None, False, "statuses")
        check_exact(ctx, i0, i1, xy, (0, 0), 7, 1, None, False, "statuses, R 1")
        p0, p1, pxy = periodic_pair16()
        ctx.set_images(p0, p1)
        check_exact(ctx, p0, p1, pxy, (0, 0), 15, 15, None, False, "ties")


# ---- 2. float pairs ----
def check_float(ctx, f0, f1, xy, off, ocw, radius, shift, swap, what, mode=0):
    """The resident pair (float images f0, f1) against the oracle: (a) surface within 1 ulp, same finite mask; (b) record and candidates
    = the oracle's tail of the device surface, bit for bit; (c) the status -3 points are the oracle's.  -> (share, worst ulp)"""
    want_rec, _, want_surf, _ = full_any(f0, f1, xy, off, ocw, radius, 0, shift=shift, swap=swap)
    rec, none, surf = ctx.match_ncc_full_any(xy, off, ocw, radius, 0, shift=shift, swap=swap, mode=mode, surface=True)
    assert none is None and ctx.last_path() == G
    st3 = want_rec[:, 2] == -3
    assert np.array_equal(rec[:, 2] == -3, st3), what + ": status -3 points"
    assert_bits_equal(rec[st3], want_rec[st3], what + ": status -3 records")
    assert np.isnan(surf[st3]).all()
    share, worst = surface_distance(surf, want_surf, what)
    print(f"{what}: {share:.6f} of the finite cells differ from the oracle, at most {worst} ulp")
    assert worst <= 1, f"{what}: a cell {worst} ulp from the oracle"
    for npeaks in (0,) + NPEAKS:
        out, cand = ctx.match_ncc_full_any(xy, off, ocw, radius, npeaks, shift=shift, swap=swap, mode=mode)
        assert ctx.last_path() == G
        t_rec, t_cand = tail_from_surface(surf, shift, radius, npeaks, refused=st3, device_snr_order=True)
        assert_bits_equal(out, t_rec, what + f": record vs the tail of the device surface, npeaks {npeaks}")
        if npeaks:
            assert_bits_equal(cand, t_cand, what + f": candidates vs the tail of the device surface, npeaks {npeaks}")
            assert np.array_equal(cand[:, st3, 2], np.full((npeaks, int(st3.sum())), -3, np.float32))
        else:
            assert cand is None
            assert_bits_equal(out, rec, what + ": the record again")
    return share, worst


@pytest.mark.parametrize("radius", PLANES_R)
@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_float_pair(api, ocw, encoding, radius):
    c, f0, f1, shift = float_case(ocw, 0.03, radius, encoding)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            check_float(ctx, f0, f1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap,
                        f"float ocw {ocw} {encoding} R {radius} swap {swap}")


@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_float_pair_without_nulls(api, ocw):
    """The clean body: no excluded pixel in any chip or box (the grid keeps its boxes inside the image)."""
    c, f0, f1, shift = float_case(ocw, 0.0, 15, "zero")
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        check_float(ctx, f0, f1, c.xyuvav, c.offset, ocw, 15, shift, False, f"float ocw {ocw} no nulls R 15")
        check_float(ctx, f0, f1, c.xyuvav, c.offset, ocw, 7, None, False, f"float ocw {ocw} no nulls R 7 no shift")


# ---- 3. the two null rules apart ----
def test_null_rules_apart(api):
    ocw, R = APART_OCW, APART_R
    n0, m0, f1, f1i, xy = rules_apart_case()
    with api.Context(0) as ctx:
        ctx.set_images(n0, f1i)
        check_float(ctx, n0, f1i, xy, (0, 0), ocw, R, None, False, "NaN chip")
        rec, _, surf = ctx.match_ncc_full_any(xy, (0, 0), ocw, R, 0, surface=True)
        assert rec[0, 2] != -3 and np.isfinite(surf[0]).any()
        # the Inf: the cells whose window holds it are not finite, every other cell is that of the pair without it
        S = 2 * R + 1
        touched = np.zeros((S, S), bool)                               # [x][y]: window of cell (x, y) = box columns x .. x + 14, rows y .. y + 14
        bx, by = APART_INF[0] - (64 - ocw - R), APART_INF[1] - (64 - ocw - R)
        for x in range(S):
            for y in range(S):
                touched[x, y] = x <= bx <= x + 2 * ocw and y <= by <= y + 2 * ocw
        assert touched.any() and not touched.all()
        assert not np.isfinite(surf[3][touched.ravel()]).any()
        ctx.set_images(n0, f1)
        plain = ctx.match_ncc_full_any(xy, (0, 0), ocw, R, 0, surface=True)[2]
        assert np.isfinite(plain[3]).all()
        assert_bits_equal(surf[3][~touched.ravel()], plain[3][~touched.ravel()], "cells beside the Inf")
        ctx.set_images(m0, f1)
        check_float(ctx, m0, f1, xy, (0, 0), ocw, R, None, False, "-9999 chip")
        assert ctx.match_ncc_full_any(xy, (0, 0), ocw, R, 0)[0][0, 2] == -3


# ---- 4. a filtered float pair ----
@pytest.mark.parametrize("ocw", FILTERED_OCW)
def test_filtered_float_pair(api, ocw):
    radius = FILTERED_R
    c, f0, f1, shift = float_case(ocw, 0.03, radius, "zero")
    H, W = f0.shape
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for k in FILTERED_KERNELS:                                    # one gradient kernel and the Laplacian
            ctx.filter_images(None)
            ctx.filter_images(api.CLI_KERNELS[k])
            g0, g1 = ctx.get_images(H, W)
            # the fixture first (the pair as the device filtered it): the oracle's two orders within 1 ulp of each other
            a = full_any(g0, g1, c.xyuvav, c.offset, ocw, radius, 0, shift=shift, order=0)[2]
            b = full_any(g0, g1, c.xyuvav, c.offset, ocw, radius, 0, shift=shift, order=1)[2]
            assert surface_distance(b, a, f"filtered float, kernel {k}: the oracle's two orders")[1] <= 1
            check_float(ctx, g0, g1, c.xyuvav, c.offset, ocw, radius, shift, False, f"filtered float, kernel {k}, ocw {ocw}")
        ctx.filter_images(None)


# ---- 4b. a pair on which the order of the additions shows ----
@pytest.mark.parametrize("radius,encoding", [(7, "zero"), (15, "m9999_nan")])
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_wide_range_pair(api, ocw, radius, encoding):
    """Six decades of amplitude: the f64 partial sums are inexact (tests/test_full_any_cpu.py asserts it for the two large chips), so the
    kernel's order and the oracle's give different sums here, and the 1-ulp assertion of check_float is a test of the bound."""
    c, f0, f1, shift = wide_case(ocw, 0.03, radius, encoding)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            check_float(ctx, f0, f1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap,
                        f"wide ocw {ocw} {encoding} R {radius} swap {swap}")


# ---- 5. dispatch and refusals ----
def test_dispatch(api):
    with api.Context(0) as ctx:
        for bits, path in ((8, "u8_mfma_full"), (12, "u16_full"), (16, "f32i_full")):
            c, i0, i1, shift = integer_pair(bits, 16, 0.03, 7)
            ctx.set_images(i0, i1)
            for npeaks in (0, 4):
                want = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift)
                got = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, npeaks, shift=shift)
                assert ctx.last_path() == path
                assert_bits_equal(got[0], want[0], f"{bits}-bit mode 0: record")
                if npeaks:
                    assert_bits_equal(got[1], want[1], f"{bits}-bit mode 0: candidates")
            with pytest.raises(api.Mimc3Error) as e:                   # only the float kernel serves the surfaces
                ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 0, shift=shift, surface=True)
            assert e.value.code == -1
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 0, shift=shift, mode=2)
            assert e.value.code == -1
            assert_bits_equal(ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 0, shift=shift)[0],
                              ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 0, shift=shift)[0], "after the refusals")


def test_refusals(api):
    c = synth.make_small(seed=21, ocw=7)
    f0, f1 = to_float(c.i0, 1), to_float(c.i1, 2)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        xy = np.ascontiguousarray(c.xyuvav, np.float64)
        out = np.empty((c.n, 8), np.float32)
        cand = np.empty((9, c.n, 3), np.float32)
        off = np.zeros(2, np.int32)
        call = api._lib.mimc3_match_ncc_full_any
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 9, 0, 0, out, cand.ctypes.data, None) == -1         # npeaks 9
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 0, 0, out, None, None) == -1                     # cand / npeaks mismatch
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 0, 0, 0, out, cand.ctypes.data, None) == -1
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 0, 0, 2, out, None, None) == -1                     # mode 2
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 0, 0, -1, out, None, None) == -1
        for ocw, radius in ((7, 0), (7, 16), (8, 5)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full_any(c.xyuvav, (0, 0), ocw, radius, 2)
            assert e.value.code == -1
        bad = c.xyuvav.copy()
        bad[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_any(bad, (0, 0), 7, 5, 2)
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_any(c.xyuvav, (300, 0), 7, 5, 2)
        assert e.value.code == -2
        rec, _ = ctx.match_ncc_full_any(c.xyuvav, (0, 0), 7, 5, 0)                                       # the pair itself is taken ...
        assert ctx.last_path() == G
        for older in (ctx.match_ncc_full_dn, ctx.match_ncc_full_planes):                                 # ... and the older entries still refuse it
            with pytest.raises(api.Mimc3Error) as e:
                older(c.xyuvav, (0, 0), 7, 5, 2)
            assert e.value.code == -6
        assert_bits_equal(ctx.match_ncc_full_any(c.xyuvav, (0, 0), 7, 5, 0)[0], rec, "the pair again, after the refusals")


# ---- 6. the _dev entry, determinism ----
def test_dev_entry_on_a_stream(api):
    import ctypes as C
    import hipmem
    from hipmem import DevArray
    c, f0, f1, shift = float_case(16, 0.03, 7, "nan_zero")
    S2 = 15 * 15
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=np.ascontiguousarray(shift, np.int32))
        d_out, d_cand, d_surf = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32), DevArray((c.n, S2), np.float32)
        d_rec = DevArray((c.n, 8), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        # (a fresh pair: the _dev entry builds the planes itself)
        ctx.match_ncc_full_any_dev(d_xy.ptr, c.n, c.offset, 16, 7, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, stream=st.value, d_surf=d_surf.ptr)
        ctx.match_ncc_full_any_dev(d_xy.ptr, c.n, c.offset, 16, 7, 0, d_rec.ptr, 0, d_shift=d_sh.ptr, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == G
        out, cand, surf = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 4, shift=shift, surface=True)
        out2, cand2, surf2 = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 4, shift=shift, surface=True)
        assert_bits_equal(out2, out, "two identical calls: record")
        assert_bits_equal(cand2, cand, "two identical calls: candidates")
        assert_bits_equal(surf2, surf, "two identical calls: surface")
        assert_bits_equal(d_out.numpy(), out, "_dev: record")
        assert_bits_equal(d_cand.numpy(), cand, "_dev: candidates")
        assert_bits_equal(d_surf.numpy(), surf, "_dev: surface")
        assert_bits_equal(d_rec.numpy(), out, "_dev: record alone")
        assert hipmem._hip.hipStreamDestroy(st) == 0


# ---- 7. full_candidates on a float pair ----
def test_full_candidates_on_a_float_pair(api):
    c, f0, f1, shift = float_case(16, 0.03, 7, "nan_zero")
    vec_ocw, npeaks = (7, 16), 2
    kernels = (None,) + api.CLI_KERNELS
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        with pytest.raises(api.Mimc3Error) as e:
            ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, 7, npeaks, shift=shift)            # the default keeps today's calls
        assert e.value.code == -6
        before = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 0, shift=shift)[0]
        dp = ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, 7, npeaks, shift=shift, any_pair=True)
        assert dp.shape == (len(kernels) * len(vec_ocw) * npeaks, c.n, 3) and dp.dtype == np.float32
        assert_bits_equal(ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 7, 0, shift=shift)[0], before, "the pair matches raw again")
        b = 0
        for v, k in enumerate(kernels):
            ctx.filter_images(None)
            ctx.filter_images(k)
            for ocw in vec_ocw:
                want = ctx.match_ncc_full_any(c.xyuvav, c.offset, ocw, 7, npeaks, shift=shift)[1]
                assert ctx.last_path() == G
                assert_bits_equal(dp[b:b + npeaks], want, f"block (variant {v}, ocw {ocw})")
                b += npeaks
        ctx.filter_images(None)
        assert (dp[:, :, 2] >= -1).mean() > 0.5
