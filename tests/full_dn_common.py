"""Test infrastructure of the exhaustive search on integral-f32 pairs (mimc3_match_ncc_full_dn): the test-side oracle on float pixels
(tests/full_dn_oracle.c), compiled on first use into tests/_build with the flags tests/full_search_common.py uses, and the 16-bit
fixtures the CPU and GPU tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from full_multi_common import STATUS_R, parity_case, periodic_pair, status_case
from full_search_common import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "full_dn_oracle.c")
LIB = os.path.join(HERE, "_build", "libfull_dn_oracle.so")
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = "%s.%d" % (LIB, os.getpid())
            subprocess.check_call(["gcc", *FLAGS, "-o", tmp, SRC, "-lm"])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.full_dn.argtypes = [_f32p, _f32p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_int, _f32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.full_dn.restype = C.c_int
        _lib = lib
    return _lib


def full_dn(i0, i1, xyuvav, offset, ocw, radius, npeaks, shift=None, swap=False, exact=False, with_counts=False, with_surface=False,
            nthreads=0):
    """The exhaustive search on float pixels on the CPU -> (float32[N][8] record, float32[npeaks][N][3] candidates or None at npeaks 0),
    then, if asked for, the number of local maxima per point (with_counts) and every point's surface float32[N][S * S] in k order
    (with_surface; NaN where the validity rule refuses the point).  exact: exact products instead of the reference's rounded ones."""
    i0 = np.ascontiguousarray(i0, np.float32)
    i1 = np.ascontiguousarray(i1, np.float32)
    xy = np.ascontiguousarray(xyuvav, np.float64)
    H, W = i0.shape
    n = xy.shape[0]
    S = 2 * radius + 1
    out = np.empty((n, 8), np.float32)
    cand = np.empty((npeaks, n, 3), np.float32) if npeaks > 0 else None
    nlm = np.empty(n, np.int32)
    surf = np.empty((n, S * S), np.float32) if with_surface else None
    sh = None if shift is None else np.ascontiguousarray(shift, np.int32)
    rc = _load().full_dn(i0, i1, H, W, xy, n, int(offset[0]), int(offset[1]), None if sh is None else sh.ctypes.data, ocw, radius,
                         npeaks, 1 if swap else 0, 1 if exact else 0, out, None if cand is None else cand.ctypes.data, nlm.ctypes.data,
                         None if surf is None else surf.ctypes.data, nthreads)
    if rc != 0:
        raise ValueError(f"full_dn rc={rc}")
    res = (out, cand)
    if with_counts:
        res += (nlm,)
    if with_surface:
        res += (surf,)
    return res


# ---- 16-bit fixtures.  A pair whose pixels are multiples of 256 has exact f32 products (16 significant bits), and a kernel that never
#      rounds a product would pass on it: every fixture here carries full low-order entropy (tests/test_full_dn_cpu.py asserts that the
#      rounded and the exact cell differ on at least a quarter of the cells of each) ----
def to_dn16(img, seed):
    """An 8-bit image (0 = null) -> 16-bit DN: 256 * pixel + 8 random low bits; nulls stay 0, the maximum is <= 65535."""
    img = np.asarray(img, np.float32)
    low = np.random.default_rng(seed).integers(0, 256, img.shape).astype(np.float32)
    out = np.where(img == 0, np.float32(0), img * np.float32(256) + low).astype(np.float32)
    assert out.max() <= 65535 and out.max() > 4095 and ((out == 0) == (img == 0)).all()
    return np.ascontiguousarray(out)


def dn16_case(ocw, null_frac, radius, dimx=5, dimy=4):
    """full_multi_common.parity_case's pair and grid as 16-bit DN -> (case, i0, i1, a-priori shift)"""
    c, shift = parity_case(ocw, null_frac, radius, dimx=dimx, dimy=dimy)
    return c, to_dn16(c.i0, 1000 + ocw), to_dn16(c.i1, 2000 + ocw), shift


def status_case16():
    """full_planes_common.status_case12's points on 16-bit values: -3, -2 (a flat chip: the low bits stay off it), -4, three points that
    overhang the image edge, a null in the chip alone (6), one in the chip and one in the box (7).  -> (i0, i1, xyuvav); ocw 7, R = STATUS_R"""
    b0, b1, xy = status_case()
    flat = b0 == 9
    i0, i1 = to_dn16(b0, 31), to_dn16(b1, 32)
    i0[flat] = 9 * 256 + 77
    xy = np.concatenate([xy, np.zeros((2, 6))])
    xy[6, 2:4] = [90, 40]
    xy[7, 2:4] = [60, 100]
    i0[40, 90] = 0
    i0[100, 60] = 0
    i1[95, 55] = 0
    return i0, i1, xy


def periodic_pair16(pu=6, pv=6):
    """An exactly periodic 16-bit pair without nulls (i0 == i1, period pu x pv px, full low-order entropy) and six grid points: offsets a
    period apart see the same pixel pairs, i.e. the same rounded products and bit-equal NCC."""
    _, _, xy = periodic_pair(pu, pv, plateau=False)
    tile = np.random.default_rng(77).integers(256, 65536, (pv, pu))
    B = np.tile(tile, (200 // pv + 2, 200 // pu + 2))[:200, :200].astype(np.float32)
    return np.ascontiguousarray(B), B.copy(), xy


def differing_fraction(i0, i1, xy, offset, ocw, radius, shift=None, swap=False):
    """Of the finite cells of the points' surfaces, the fraction whose f32 bits differ between rounded and exact products."""
    a = full_dn(i0, i1, xy, offset, ocw, radius, 0, shift=shift, swap=swap, with_surface=True)[2]
    b = full_dn(i0, i1, xy, offset, ocw, radius, 0, shift=shift, swap=swap, exact=True, with_surface=True)[2]
    ok = np.isfinite(a) & np.isfinite(b)
    return float((a.view(np.uint32)[ok] != b.view(np.uint32)[ok]).mean()) if ok.any() else 0.0


def c2_dn16():
    """BASELINE C2 (4096^2, 200,000 points) as full-entropy 16-bit DN -> (case, i0, i1)"""
    from mimc3_amd import synth
    c = synth.make_case("C2")
    return c, to_dn16(c.i0, 5), to_dn16(c.i1, 6)


C2_SAMPLE = 20000


def c2_sample(n):
    """the fixed-seed sample of C2's points the full-size test compares, ascending"""
    sel = np.random.default_rng(2).choice(n, C2_SAMPLE, replace=False)
    sel.sort()
    return sel
