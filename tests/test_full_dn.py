"""GPU: the exhaustive search on every pair the planes' matchers take (mimc3_match_ncc_full_dn) -- 16-bit DN and its filtered forms on the
f32 planes against the test-side oracle on float pixels (tests/full_dn_oracle.c: the reference's rounded f32 products), 8-bit and
12-bit pairs against the entries that took them before.  Every comparison is on the bit patterns (NaN == NaN), every point is
compared; the SNR as tests/full_search_common.py compares it (its f64 sum runs in another order on the device)."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_dn_common import (c2_dn16, c2_sample, differing_fraction, dn16_case, full_dn, periodic_pair16, status_case16)
from full_multi_common import STATUS_R, parity_case
from full_planes_common import PLANES_OCW, PLANES_R, dn12_case, null_sides
from full_search_common import assert_records_match
from mimc3_amd import synth

pytestmark = pytest.mark.gpu

NPEAKS = (1, 4, 8)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_against_oracle(ctx, f0, f1, xy, off, ocw, radius, shift, swap, what, path="f32i_full"):
    """Record (npeaks 0) and candidates (npeaks 1, 4, 8) of the resident pair against the oracle on the float images f0, f1."""
    want_rec, want = full_dn(f0, f1, xy, off, ocw, radius, 8, shift=shift, swap=swap)
    rec, none = ctx.match_ncc_full_dn(xy, off, ocw, radius, 0, shift=shift, swap=swap)
    assert none is None and ctx.last_path() == path
    assert_records_match(rec, want_rec, what + ": record")
    for npeaks in NPEAKS:
        out, cand = ctx.match_ncc_full_dn(xy, off, ocw, radius, npeaks, shift=shift, swap=swap)
        assert ctx.last_path() == path and cand.shape == (npeaks, xy.shape[0], 3)
        assert_bits_equal(out, rec, what + f": record at npeaks {npeaks} vs npeaks 0")
        assert_bits_equal(cand, want[:npeaks], what + f": candidates, npeaks {npeaks}")
    return want_rec, want


@pytest.mark.parametrize("radius", PLANES_R)
@pytest.mark.parametrize("null_frac", [0.0, 0.03])
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_16bit_pair(api, ocw, null_frac, radius):
    c, i0, i1, shift = dn16_case(ocw, null_frac, radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            check_against_oracle(ctx, i0, i1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap,
                                 f"16-bit ocw {ocw} nulls {null_frac} R {radius} swap {swap}")
        check_against_oracle(ctx, i0, i1, c.xyuvav, c.offset, ocw, radius, None, False, f"16-bit ocw {ocw} R {radius} no shift")


@pytest.mark.parametrize("radius", PLANES_R)
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_filtered_16bit_pair(api, ocw, radius):
    """The three CLI kernels on fresh planes each.  The oracle reads ctx.get_images() as they are: integers for the gradients (shift 0),
    multiples of 1/8 for the Laplacian (shift 3).  The filtered pairs must tell rounded from exact products too."""
    c, i0, i1, shift = dn16_case(ocw, 0.03, radius)
    H, W = i0.shape
    seen = set()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for k, kern in enumerate(api.CLI_KERNELS):
            ctx.filter_images(None)                               # fresh planes: what a filter leaves in the border is the next one's input
            ctx.filter_images(kern)
            f0, f1 = ctx.get_images(H, W)
            q0, q1 = f0 * np.float32(8), f1 * np.float32(8)
            assert (q0 == np.rint(q0)).all() and (q1 == np.rint(q1)).all() and min(q0.min(), q1.min()) >= 0
            integral = bool((f0 == np.rint(f0)).all() and (f1 == np.rint(f1)).all())
            assert max(q0.max(), q1.max()) >= 8 * 4096 and max((f0 if integral else q0).max(), (f1 if integral else q1).max()) < 2 ** 20
            seen.add("shift0" if integral else "shift3")
            assert differing_fraction(f0, f1, c.xyuvav, c.offset, ocw, radius, shift=shift) >= 0.25
            for swap in (False, True):
                sgn = -1 if swap else 1
                check_against_oracle(ctx, f0, f1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap,
                                     f"kernel {k} ocw {ocw} R {radius} swap {swap}")
        ctx.filter_images(None)
    assert {"shift0", "shift3"} <= seen, seen


def test_nulls_and_statuses(api):
    i0, i1, xy = status_case16()
    want_out, want, nlm = full_dn(i0, i1, xy, (0, 0), 7, STATUS_R, 4, with_counts=True)
    st = want_out[:, 2]
    assert (st == -2).any() and (st == -3).any() and (st == -4).any()
    sides = null_sides(i0, i1, xy, 7, STATUS_R)
    assert any(c > 0 and b == 0 for c, b in sides) and any(c == 0 and b > 0 for c, b in sides) and any(c > 0 and b > 0 for c, b in sides)
    assert ((nlm < 4) & (st != -3)).any()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check_against_oracle(ctx, i0, i1, xy, (0, 0), 7, STATUS_R, None, False, "statuses")
        check_against_oracle(ctx, i0, i1, xy, (0, 0), 7, 1, None, False, "statuses, R 1")
        # a planted tie: an exactly periodic 16-bit pair -- 25 bit-equal interior peaks ranked by k
        p0, p1, pxy = periodic_pair16()
        ctx.set_images(p0, p1)
        _, tied = check_against_oracle(ctx, p0, p1, pxy, (0, 0), 15, 15, None, False, "ties")
        assert all(len(set(tied[:, g, 2].view(np.uint32).tolist())) == 1 for g in range(pxy.shape[0]))


def test_8bit_and_12bit_pairs_through_the_new_entry(api):
    c, shift = parity_case(16, 0.03, 7)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        rec, none = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 0, shift=shift)
        assert none is None and ctx.last_path() == "u8_mfma_full"
        assert_bits_equal(rec, ctx.match_ncc_full(c.xyuvav, c.offset, 16, 7, shift=shift), "record vs match_ncc_full")
        out, cand = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 4, shift=shift)
        assert ctx.last_path() == "u8_mfma_full"
        o2, c2 = ctx.match_ncc_full_multi(c.xyuvav, c.offset, 16, 7, 4, shift=shift)
        assert_bits_equal(out, o2, "record vs match_ncc_full_multi")
        assert_bits_equal(cand, c2, "candidates vs match_ncc_full_multi")
        c, i0, i1, shift = dn12_case(16, 0.03, 7)
        ctx.set_images(i0, i1)
        for npeaks in (0, 4):
            for swap in (False, True):
                sgn = -1 if swap else 1
                got = ctx.match_ncc_full_dn(c.xyuvav, sgn * c.offset, 16, 7, npeaks, shift=sgn * shift, swap=swap)
                assert ctx.last_path() == "u16_full"
                old = ctx.match_ncc_full_planes(c.xyuvav, sgn * c.offset, 16, 7, npeaks, shift=sgn * shift, swap=swap)
                assert ctx.last_path() == "u16_full"
                assert_bits_equal(got[0], old[0], f"12-bit record vs match_ncc_full_planes, npeaks {npeaks} swap {swap}")
                if npeaks:
                    assert_bits_equal(got[1], old[1], f"12-bit candidates vs match_ncc_full_planes, swap {swap}")
                else:
                    assert got[1] is None and old[1] is None


def test_refusals(api):
    c = synth.make_small(seed=21, ocw=7)
    i0 = (c.i0 * 256 + 3 * (c.i0 > 0)).astype(np.float32)
    i1 = (c.i1 * 256 + 5 * (c.i1 > 0)).astype(np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        xy = np.ascontiguousarray(c.xyuvav, np.float64)
        out = np.empty((c.n, 8), np.float32)
        cand = np.empty((9, c.n, 3), np.float32)
        off = np.zeros(2, np.int32)
        call = api._lib.mimc3_match_ncc_full_dn
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 9, 0, out, cand.ctypes.data) == -1            # npeaks 9
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 0, out, None) == -1                        # cand / npeaks mismatch
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 0, 0, out, cand.ctypes.data) == -1
        for ocw, radius in ((7, 0), (7, 16), (8, 5)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full_dn(c.xyuvav, (0, 0), ocw, radius, 2)
            assert e.value.code == -1
        bad = c.xyuvav.copy()
        bad[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_dn(bad, (0, 0), 7, 5, 2)
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_dn(c.xyuvav, (300, 0), 7, 5, 2)
        assert e.value.code == -2
        rec, _ = ctx.match_ncc_full_dn(c.xyuvav, (0, 0), 7, 5, 0)                                   # the pair itself is taken ...
        assert ctx.last_path() == "f32i_full"
        with pytest.raises(api.Mimc3Error) as e:                                                    # ... and the older entry still refuses it
            ctx.match_ncc_full_planes(c.xyuvav, (0, 0), 7, 5, 2)
        assert e.value.code == -6
        n0 = i0.copy()
        n0[n0 == 0] = np.nan
        n0[5, 5] = np.nan
        ctx.set_images(n0, i1)                                                                      # NaN nulls
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_dn(c.xyuvav, (0, 0), 7, 5, 0)
        assert e.value.code == -6
        h0 = i0.copy()
        h0[9, 9] += np.float32(0.3)                                                                 # (not a multiple of 1/8)
        ctx.set_images(h0, i1)                                                                      # a non-integral pair
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_dn(c.xyuvav, (0, 0), 7, 5, 4)
        assert e.value.code == -6
        ctx.set_images(i0, i1)
        assert_bits_equal(ctx.match_ncc_full_dn(c.xyuvav, (0, 0), 7, 5, 0)[0], rec, "the pair again, after the refusals")


def test_dev_entry_on_a_stream(api):
    import ctypes as C
    import hipmem
    from hipmem import DevArray
    c, i0, i1, shift = dn16_case(16, 0.03, 7)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 4, shift=shift)
        rec, _ = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 0, shift=shift)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=np.ascontiguousarray(shift, np.int32))
        d_out, d_cand, d_rec = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32), DevArray((c.n, 8), np.float32)
        st = C.c_void_p()                                       # a stream of the runtime the library runs on
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_full_dn_dev(d_xy.ptr, c.n, c.offset, 16, 7, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, stream=st.value)
        ctx.match_ncc_full_dn_dev(d_xy.ptr, c.n, c.offset, 16, 7, 0, d_rec.ptr, 0, d_shift=d_sh.ptr, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == "f32i_full"
        assert_bits_equal(d_out.numpy(), out, "_dev: record")
        assert_bits_equal(d_cand.numpy(), cand, "_dev: candidates")
        assert_bits_equal(d_rec.numpy(), rec, "_dev: record alone")
        assert hipmem._hip.hipStreamDestroy(st) == 0


def test_dev_entry_builds_the_planes_itself(api):
    """A fresh pair whose first search call is the _dev entry on a caller's stream: the planes and tables are built before it enqueues."""
    import ctypes as C
    import hipmem
    from hipmem import DevArray
    c, i0, i1, shift = dn16_case(7, 0.03, 7)
    want_out, want = full_dn(i0, i1, c.xyuvav, c.offset, 7, 7, 4, shift=shift)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=np.ascontiguousarray(shift, np.int32))
        d_out, d_cand = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_full_dn_dev(d_xy.ptr, c.n, c.offset, 7, 7, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert_records_match(d_out.numpy(), want_out, "_dev first: record")
        assert_bits_equal(d_cand.numpy(), want, "_dev first: candidates")
        assert hipmem._hip.hipStreamDestroy(st) == 0


def test_full_candidates_on_a_16bit_pair(api):
    c, i0, i1, shift = dn16_case(16, 0.03, 7)
    vec_ocw, npeaks = (7, 16), 2
    kernels = (None,) + api.CLI_KERNELS
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        before = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 0, shift=shift)[0]
        dp = ctx.full_candidates(c.xyuvav, c.offset, vec_ocw, 7, npeaks, shift=shift)
        assert dp.shape == (len(kernels) * len(vec_ocw) * npeaks, c.n, 3) and dp.dtype == np.float32
        assert_bits_equal(ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 7, 0, shift=shift)[0], before, "the pair matches raw again")
        b = 0
        for v, k in enumerate(kernels):
            ctx.filter_images(None)
            ctx.filter_images(k)
            for ocw in vec_ocw:
                want = ctx.match_ncc_full_dn(c.xyuvav, c.offset, ocw, 7, npeaks, shift=shift)[1]
                assert ctx.last_path() == "f32i_full"
                assert_bits_equal(dp[b:b + npeaks], want, f"block (variant {v}, ocw {ocw})")
                b += npeaks
        ctx.filter_images(None)
        assert (dp[:, :, 2] >= -1).mean() > 0.5


def test_full_size_c2_16bit_sample(api):
    """C2 (4096^2, 200,000 points, ocw 16, R 15, centred on the a-priori shift) as full-entropy 16-bit DN, npeaks 4: the whole pass on the
    device, a 20,000-point sample (fixed seed) against the oracle."""
    c, i0, i1 = c2_dn16()
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 15, 4, shift=shift)
        assert ctx.last_path() == "f32i_full"
        rec, _ = ctx.match_ncc_full_dn(c.xyuvav, c.offset, 16, 15, 0, shift=shift)
    assert_bits_equal(out, rec, "record at npeaks 4 vs npeaks 0")
    sel = c2_sample(c.n)
    want_out, want = full_dn(i0, i1, c.xyuvav[sel], c.offset, 16, 15, 4, shift=shift[sel])
    assert_bits_equal(cand[:, sel], want, "C2 16-bit sample: candidates")
    assert_records_match(out[sel], want_out, "C2 16-bit sample: record")
    fit = out[:, 2] >= -1
    assert fit.mean() > 0.9
    assert_bits_equal(cand[0][fit], out[fit, :3], "candidate 0 vs the record")
