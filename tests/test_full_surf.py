"""GPU: the surfaces from the integer-class kernels (mimc3_match_ncc_full_surf; the SURF forms of match_mx_kernel.hip,
match_full_u16_kernel.hip and match_full_f32_kernel.hip).

On 8-bit, 12-bit and 16-bit pairs the entry returns match_ncc_full_dn's record and candidates bit for bit from that class's own kernel,
and a surface that equals the float kernel's (match_ncc_full_any(mode=1, surface=True)) and the float oracle's under the contract of
include/mimc3_hip.h: the same f32 value in every cell -- finite cells bit for bit, a non-finite cell of the same kind; NaN payloads are
not part of it.  Byte equality is tried first and its outcome printed per case (python -m pytest -s); the assertion is the contract.
Every null fixture holds at least two points of every form its kernel distinguishes (counted on the CPU, asserted here), so every form
must store."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import FILTERED_KERNELS, float_case, full_any
from full_dn_common import periodic_pair16, status_case16
from full_multi_common import STATUS_R, periodic_pair, status_case
from full_surf_common import BITS, PATH, SURF_OCW, SURF_R, class_counts, every_form_stores, null_classes, surf_case, surfaces_equal

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
G = "f32g_full"


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_surf(ctx, path, i0, i1, xy, off, ocw, radius, shift, swap, what):
    """The resident integer-class pair: record and candidates against match_ncc_full_dn, the surface against the float kernel and the
    float oracle.  -> (record, surface)"""
    want_surf = full_any(i0, i1, xy, off, ocw, radius, 0, shift=shift, swap=swap)[2]
    ref_rec, _ = ctx.match_ncc_full_dn(xy, off, ocw, radius, 0, shift=shift, swap=swap)
    assert ctx.last_path() == path
    _, _, float_surf = ctx.match_ncc_full_any(xy, off, ocw, radius, 0, shift=shift, swap=swap, mode=1, surface=True)
    assert ctx.last_path() == G
    rec, none, surf = ctx.match_ncc_full_surf(xy, off, ocw, radius, 0, shift=shift, swap=swap)
    assert none is None and ctx.last_path() == path
    assert_bits_equal(rec, ref_rec, what + ": record vs match_ncc_full_dn")
    same = surfaces_equal(surf, float_surf, what + ": surface vs the float kernel")
    print(f"{what}: surface bytes {'equal' if same else 'NOT equal (NaN payloads)'} to the float kernel's")
    surfaces_equal(surf, want_surf, what + ": surface vs the oracle")
    assert np.isnan(surf[rec[:, 2] == -3]).all(), what + ": a status -3 point has an all-NaN surface"
    for npeaks in (1, 8):
        ref_out, ref_cand = ctx.match_ncc_full_dn(xy, off, ocw, radius, npeaks, shift=shift, swap=swap)
        out, cand, surf_k = ctx.match_ncc_full_surf(xy, off, ocw, radius, npeaks, shift=shift, swap=swap)
        assert ctx.last_path() == path and cand.shape == (npeaks, xy.shape[0], 3)
        assert_bits_equal(out, ref_out, what + f": record, npeaks {npeaks}")
        assert_bits_equal(cand, ref_cand, what + f": candidates, npeaks {npeaks}")
        surfaces_equal(surf_k, surf, what + f": surface at npeaks {npeaks} vs npeaks 0")
    return rec, surf


# ---- 1. every class, every form, the chip sizes and radii at which the store can go wrong ----
@pytest.mark.parametrize("radius", SURF_R)
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("ocw", SURF_OCW)
@pytest.mark.parametrize("bits", BITS)
def test_surfaces_on_integer_pairs(api, bits, ocw, nulls, radius):
    c, i0, i1, shift = surf_case(bits, ocw, nulls, radius)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            off, sh = sgn * c.offset, sgn * shift
            cls = null_classes(i0, i1, c.xyuvav, off, sh, ocw, radius, swap)
            what = f"{bits}-bit ocw {ocw} nulls {nulls} R {radius} swap {swap} classes {class_counts(cls)}"
            if nulls:
                assert every_form_stores(bits, cls), what + ": a form of the kernel finishes fewer than 2 points"
            else:
                assert class_counts(cls)[0] == c.n, what
            rec, surf = check_surf(ctx, PATH[bits], i0, i1, c.xyuvav, off, ocw, radius, sh, swap, what)
            for k in range(3):                                   # every form left a surface with finite cells
                sel = (cls == k) & (rec[:, 2] != -3)
                if (cls == k).any() and nulls:
                    assert sel.any() and np.isfinite(surf[sel]).any(axis=1).all(), what + f": form {k}"
        rec, surf = check_surf(ctx, PATH[bits], i0, i1, c.xyuvav, c.offset, ocw, radius, None, False,
                               f"{bits}-bit ocw {ocw} nulls {nulls} R {radius} no shift")


# ---- 2. statuses, ties ----
@pytest.mark.parametrize("bits", (8, 16))
def test_statuses_and_ties(api, bits):
    i0, i1, xy = status_case() if bits == 8 else status_case16()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for radius in (STATUS_R, 1):
            rec, surf = check_surf(ctx, PATH[bits], i0, i1, xy, (0, 0), 7, radius, None, False, f"{bits}-bit statuses R {radius}")
            if radius == STATUS_R:
                st = rec[:, 2]
                assert (st == -2).any() and (st == -3).any() and (st == -4).any()
                assert np.isnan(surf[st == -3]).all() and np.isnan(rec[st == -3][:, [0, 1, 3, 4, 5, 6, 7]]).all()
        if bits == 8:
            p0, p1, pxy = periodic_pair(6, 6, plateau=False)
            ctx.set_images(p0, p1)
            rec, surf = check_surf(ctx, PATH[8], p0, p1, pxy, (0, 0), 15, 15, None, False, "8-bit ties")
            S = 31
            ties = [(su + 15) * S + (sv + 15) for su in (-12, -6, 0, 6, 12) for sv in (-12, -6, 0, 6, 12)]
            assert (surf[:, ties] == surf[:, ties[:1]]).all()                  # offsets a period apart: bit-equal cells
            p0, p1, pxy = periodic_pair(3, 3, plateau=True)
            ctx.set_images(p0, p1)
            check_surf(ctx, PATH[8], p0, p1, pxy, (0, 0), 7, 4, None, False, "8-bit plateau")
        else:
            p0, p1, pxy = periodic_pair16()
            ctx.set_images(p0, p1)
            check_surf(ctx, PATH[16], p0, p1, pxy, (0, 0), 15, 15, None, False, "16-bit ties")


# ---- 3. point order, bounds and the end of the buffer: the _dev entry on a stream of its own ----
@pytest.mark.parametrize("ocw,radius", [(16, 15), (7, 4)])
@pytest.mark.parametrize("bits", BITS)
def test_dev_entry_point_order_and_bounds(api, bits, ocw, radius):
    """N = 20 or 42: not a multiple of 8, so the launch is rounded up and the XCD-contiguous order permutes the points.  Point 5's chip
    leaves the image and point 11's search box leaves the zero border: the host entry refuses such a call, the kernels give both an
    all-NaN record and surface.  Behind [N][S^2] the surface buffer holds a sentinel, which must come back untouched."""
    import hipmem
    from hipmem import DevArray
    c, i0, i1, shift = surf_case(bits, ocw, True, radius)
    n, S2, TAIL, SENT = c.n, (2 * radius + 1) ** 2, 4096, np.float32(-12345.5)
    assert n > 8 and n % 8 != 0
    xy = np.ascontiguousarray(c.xyuvav).copy()
    sh = np.ascontiguousarray(shift, np.int32).copy()
    xy[5, 2] = 3.0
    sh[11] = (100000, 0)
    bad = np.zeros(n, bool)
    bad[[5, 11]] = True
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        d_xy, d_sh = DevArray(src=xy), DevArray(src=sh)
        fill = np.full(n * S2 + TAIL, SENT, np.float32)
        d_surf, d_fsurf = DevArray(src=fill), DevArray((n, S2), np.float32)
        d_out, d_cand = DevArray((n, 8), np.float32), DevArray((4, n, 3), np.float32)
        d_ref, d_rcand, d_frec = DevArray((n, 8), np.float32), DevArray((4, n, 3), np.float32), DevArray((n, 8), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_full_surf_dev(d_xy.ptr, n, c.offset, ocw, radius, 4, d_out.ptr, d_surf.ptr, d_cand=d_cand.ptr, d_shift=d_sh.ptr,
                                    stream=st.value)
        assert ctx.last_path() == PATH[bits]
        ctx.match_ncc_full_dn_dev(d_xy.ptr, n, c.offset, ocw, radius, 4, d_ref.ptr, d_rcand.ptr, d_shift=d_sh.ptr, stream=st.value)
        ctx.match_ncc_full_any_dev(d_xy.ptr, n, c.offset, ocw, radius, 0, d_frec.ptr, 0, d_shift=d_sh.ptr, stream=st.value, mode=1,
                                   d_surf=d_fsurf.ptr)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        what = f"{bits}-bit ocw {ocw} R {radius} _dev"
        got = d_surf.numpy()
        assert (got[n * S2:] == SENT).all(), what + ": the tail behind [N][S^2] was written"
        surf, out, cand = got[:n * S2].reshape(n, S2), d_out.numpy(), d_cand.numpy()
        assert not (surf == SENT).any(), what + ": a cell was never written"
        assert_bits_equal(out, d_ref.numpy(), what + ": record vs match_ncc_full_dn_dev")
        assert_bits_equal(cand, d_rcand.numpy(), what + ": candidates vs match_ncc_full_dn_dev")
        same = surfaces_equal(surf, d_fsurf.numpy(), what + ": surface vs the float kernel")
        print(f"{what}: surface bytes {'equal' if same else 'NOT equal (NaN payloads)'} to the float kernel's")
        assert np.isnan(out[bad]).all() and np.isnan(surf[bad]).all() and np.isnan(cand[:, bad, :2]).all(), what + ": the two bad points"
        assert np.isfinite(surf[~bad]).any(axis=1).sum() >= n // 2
        # the good points are the host entry's: the call without the two bad points
        rec_h, cand_h, surf_h = ctx.match_ncc_full_surf(xy[~bad], c.offset, ocw, radius, 4, shift=sh[~bad])
        assert_bits_equal(out[~bad], rec_h, what + ": the good points' records vs the host entry")
        assert_bits_equal(cand[:, ~bad], cand_h, what + ": the good points' candidates vs the host entry")
        surfaces_equal(surf[~bad], surf_h, what + ": the good points' surfaces vs the host entry")
        assert hipmem._hip.hipStreamDestroy(st) == 0


# ---- 4. dispatch and refusals ----
def test_float_pair_goes_to_the_float_kernel(api):
    c, f0, f1, shift = float_case(16, 0.03, 4, "nan_zero")
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for npeaks in (0, 4):
            want = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 4, npeaks, shift=shift, mode=0, surface=True)
            assert ctx.last_path() == G
            got = ctx.match_ncc_full_surf(c.xyuvav, c.offset, 16, 4, npeaks, shift=shift)
            assert ctx.last_path() == G
            assert_bits_equal(got[0], want[0], f"float pair, npeaks {npeaks}: record")
            assert surfaces_equal(got[2], want[2], f"float pair, npeaks {npeaks}: surface"), "the same kernel: the same bytes"
            if npeaks:
                assert_bits_equal(got[1], want[1], "float pair: candidates")


def test_filtered_8bit_pair_goes_to_the_u16_kernel(api):
    c, i0, i1, shift = surf_case(8, 16, True, 4)
    H, W = i0.shape
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.filter_images(api.CLI_KERNELS[FILTERED_KERNELS[1]])           # the Laplacian: multiples of 1/8, u16 planes at shift 3
        g0, g1 = ctx.get_images(H, W)
        check_surf(ctx, "u16_full", g0, g1, c.xyuvav, c.offset, 16, 4, shift, False, "filtered 8-bit pair")
        ctx.filter_images(None)
        check_surf(ctx, PATH[8], i0, i1, c.xyuvav, c.offset, 16, 4, shift, False, "the pair raw again")


def test_refusals(api):
    c, i0, i1, shift = surf_case(8, 7, False, 4)
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    off = np.ascontiguousarray(c.offset, np.int32)
    out, cand = np.empty((c.n, 8), np.float32), np.empty((9, c.n, 3), np.float32)
    surf = np.empty((c.n, 33 * 33), np.float32)
    call = api._lib.mimc3_match_ncc_full_surf
    with api.Context(0) as ctx:
        assert call(ctx._h, xy, c.n, off, None, 7, 4, 0, 0, out, None, surf.ctypes.data) == ESTATE      # before set_images
        assert call(ctx._h, xy, c.n, off, None, 7, 4, 0, 0, out, None, None) == EINVAL                  # (arguments come first)
        ctx.set_images(i0, i1)
        before = ctx.match_ncc_full_surf(c.xyuvav, c.offset, 7, 4, 4, shift=shift)
        assert call(ctx._h, xy, c.n, off, None, 7, 4, 0, 0, out, None, None) == EINVAL                  # surf missing
        assert call(ctx._h, xy, c.n, off, None, 7, 16, 0, 0, out, None, surf.ctypes.data) == EINVAL     # R 16
        assert call(ctx._h, xy, c.n, off, None, 7, 0, 0, 0, out, None, surf.ctypes.data) == EINVAL      # R 0
        assert call(ctx._h, xy, c.n, off, None, 7, 4, 9, 0, out, cand.ctypes.data, surf.ctypes.data) == EINVAL      # npeaks 9
        assert call(ctx._h, xy, c.n, off, None, 7, 4, 2, 0, out, None, surf.ctypes.data) == EINVAL      # cand goes with npeaks
        assert call(ctx._h, xy, c.n, off, None, 8, 4, 0, 0, out, None, surf.ctypes.data) == EINVAL      # ocw 8
        dev = api._lib.mimc3_match_ncc_full_surf_dev
        assert dev(ctx._h, 1 << 20, c.n, 0, 0, None, 7, 4, 0, 0, 1 << 20, None, None, None) == EINVAL   # _dev: d_surf missing (nothing is read)
        with pytest.raises(api.Mimc3Error) as e:                       # the older entry keeps refusing the surfaces of an integer kernel
            ctx.match_ncc_full_any(c.xyuvav, c.offset, 7, 4, 0, shift=shift, mode=0, surface=True)
        assert e.value.code == EINVAL
        after = ctx.match_ncc_full_surf(c.xyuvav, c.offset, 7, 4, 4, shift=shift)
        for a, b, name in zip(after, before, ("record", "candidates", "surface")):
            assert_bits_equal(a, b, "after the refusals: " + name)
