"""Test infrastructure of the exhaustive search on any f32 pair (mimc3_match_ncc_full_any): the test-side oracle on float pixels with the
reference's two null rules (tests/full_any_oracle.c), compiled on first use into tests/_build with the flags
tests/full_search_common.py uses, and the float fixtures the CPU and GPU tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from full_multi_common import parity_case
from full_search_common import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "full_any_oracle.c")
LIB = os.path.join(HERE, "_build", "libfull_any_oracle.so")
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_lib = None

ENCODINGS = ("zero", "nan_zero", "m9999_nan")


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = "%s.%d" % (LIB, os.getpid())
            subprocess.check_call(["gcc", *FLAGS, "-o", tmp, SRC, "-lm"])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.full_any.argtypes = [_f32p, _f32p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, _f32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.full_any.restype = C.c_int
        lib.tail_from_surface.argtypes = [_f32p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _f32p, C.c_void_p, C.c_void_p]
        lib.tail_from_surface.restype = C.c_int
        _lib = lib
    return _lib


def full_any(i0, i1, xyuvav, offset, ocw, radius, npeaks, shift=None, swap=False, order=0, with_sums=False, nthreads=0):
    """The exhaustive search on float pixels on the CPU, the reference's two null rules -> (float32[N][8] record, float32[npeaks][N][3]
    candidates or None at npeaks 0, float32[N][S * S] surfaces in k order (NaN where the validity rule refuses the point), int32[N]
    local-maximum counts; with_sums: then float64[N][S * S][6], every cell's n, sx, sy, sxx, syy, sxy as summed).  order 0: sums in the reference's pixel order; 1: backwards into four interleaved partial sums."""
    i0 = np.ascontiguousarray(i0, np.float32)
    i1 = np.ascontiguousarray(i1, np.float32)
    xy = np.ascontiguousarray(xyuvav, np.float64)
    H, W = i0.shape
    n = xy.shape[0]
    S = 2 * radius + 1
    out = np.empty((n, 8), np.float32)
    cand = np.empty((npeaks, n, 3), np.float32) if npeaks > 0 else None
    nlm = np.empty(n, np.int32)
    surf = np.empty((n, S * S), np.float32)
    sums = np.empty((n, S * S, 6), np.float64) if with_sums else None
    sh = None if shift is None else np.ascontiguousarray(shift, np.int32)
    rc = _load().full_any(i0, i1, H, W, xy, n, int(offset[0]), int(offset[1]), None if sh is None else sh.ctypes.data, ocw, radius,
                          npeaks, 1 if swap else 0, order, out, None if cand is None else cand.ctypes.data, nlm.ctypes.data,
                          surf.ctypes.data, None if sums is None else sums.ctypes.data, nthreads)
    if rc != 0:
        raise ValueError(f"full_any rc={rc}")
    return (out, cand, surf, nlm, sums) if with_sums else (out, cand, surf, nlm)


def tail_from_surface(surf, shift, radius, npeaks, refused=None, device_snr_order=False):
    """Record and candidates computed from given surfaces float32[N][S * S], the statements of the oracle's own tail ->
    (float32[N][8], float32[npeaks][N][3] or None).  refused: bool[N], the status -3 points (their surfaces are all NaN, as are those of
    some -2 points).  device_snr_order: add the SNR's squares in the device tail's order (64 strided partial sums, pairwise tree), which
    makes column 4 comparable bit for bit as well."""
    surf = np.ascontiguousarray(surf, np.float32)
    n = surf.shape[0]
    assert surf.shape[1] == (2 * radius + 1) ** 2
    out = np.empty((n, 8), np.float32)
    cand = np.empty((npeaks, n, 3), np.float32) if npeaks > 0 else None
    sh = None if shift is None else np.ascontiguousarray(shift, np.int32)
    rf = None if refused is None else np.ascontiguousarray(refused, np.uint8)
    rc = _load().tail_from_surface(surf, None if rf is None else rf.ctypes.data, n, None if sh is None else sh.ctypes.data, radius, npeaks,
                                   1 if device_snr_order else 0, out, None if cand is None else cand.ctypes.data, None)
    if rc != 0:
        raise ValueError(f"tail_from_surface rc={rc}")
    return out, cand


# ---- float fixtures ----
def to_float(img, seed):
    """An 8-bit image (0 = null) as non-integral floats: pixel * 0.37 + U(0, 0.37) where non-null (f32), nulls kept 0."""
    img = np.asarray(img, np.float32)
    u = np.random.default_rng(seed).random(img.shape).astype(np.float32) * np.float32(0.37)
    out = np.where(img == 0, np.float32(0), img * np.float32(0.37) + u).astype(np.float32)
    assert ((out == 0) == (img == 0)).all()
    return np.ascontiguousarray(out)


def encode_nulls(f0, f1, encoding):
    """The nulls (0) of a float pair in one of ENCODINGS: 0 in both; NaN in image 0 with 0 in image 1; -9999 in image 0 with NaN in image 1."""
    f0, f1 = f0.copy(), f1.copy()
    if encoding == "nan_zero":
        f0[f0 == 0] = np.nan
    elif encoding == "m9999_nan":
        f0[f0 == 0] = -9999.0
        f1[f1 == 0] = np.nan
    else:
        assert encoding == "zero"
    return f0, f1


def float_case(ocw, null_frac, radius, encoding="zero", dimx=5, dimy=4):
    """full_multi_common.parity_case's pair and grid as non-integral floats, nulls in `encoding` -> (case, f0, f1, a-priori shift)"""
    c, shift = parity_case(ocw, null_frac, radius, dimx=dimx, dimy=dimy)
    f0, f1 = encode_nulls(to_float(c.i0, 3000 + ocw), to_float(c.i1, 4000 + ocw), encoding)
    return c, f0, f1, shift


def wide_case(ocw, null_frac, radius, encoding="zero", dimx=5, dimy=4):
    """float_case times a smooth amplitude field 10^(3 sin(2 pi (x + 0.6 y) / 160)), the same in both images: six decades over the image,
    up to 1.7 decades inside the smallest chip on top of the texture's 2.4 -- the f32 terms of a cell span more than 2^27, so its f64
    partial sums are NOT exact and the order of the additions shows in their last bits (float_case's terms span 2^39 at most from the
    smallest to the largest SUM and stay exact: there the bound is never exercised; tests/test_full_any_cpu.py asserts both).
    -> (case, f0, f1, a-priori shift)"""
    c, f0, f1, shift = float_case(ocw, null_frac, radius, "zero", dimx=dimx, dimy=dimy)
    H, W = f0.shape
    yy, xx = np.mgrid[0:H, 0:W]
    amp = np.power(10.0, 3.0 * np.sin(2 * np.pi * (xx + 0.6 * yy) / 160.0)).astype(np.float32)
    w0, w1 = encode_nulls((f0 * amp).astype(np.float32), (f1 * amp).astype(np.float32), encoding)
    return c, np.ascontiguousarray(w0), np.ascontiguousarray(w1), shift


def null_rule_pair():
    """A 64 x 64 float pair with every kind of excluded pixel: NaN, -9999, -0.0, 1e-11 (below MIN_DN), 0; and a tiny included one (1e-9).
    Point 1's chip is NaN throughout (valid: no pixel < MIN_DN; no included pixel), point 2's the same as -9999 (refused).
    -> (i0, i1, xyuvav); ocw 7"""
    rng = np.random.default_rng(5)
    base = rng.random((64, 64)).astype(np.float32) * 50 + 1
    i0 = base + rng.random((64, 64)).astype(np.float32)
    i1 = np.roll(base, (1, -1), axis=(0, 1)) + rng.random((64, 64)).astype(np.float32)
    for img, seed in ((i0, 1), (i1, 2)):
        r = np.random.default_rng(seed)
        for value in (np.nan, -9999.0, -0.0, 1e-11, 0.0, 1e-9):
            ys, xs = r.integers(0, 64, 40), r.integers(0, 64, 40)
            img[ys, xs] = value
    i0[8:23, 8:23] = np.nan
    i0[38:53, 8:23] = -9999.0
    xy = np.zeros((4, 6))
    xy[:, 2:4] = [[40, 30], [15, 15], [15, 45], [45, 45]]
    return np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32), xy


APART_OCW, APART_R = 7, 5
APART_INF = (64 - 4, 64 + 9)            # (u, v) of the +Inf pixel of rules_apart_case's image 1


def rules_apart_case():
    """The two null rules apart, ocw APART_OCW, R APART_R, four points.  Point 0's chip has 195 of its 225 pixels (86.7 % > 80 %) marked:
    as NaN (n0) it stays valid and its cells use the 30 pixels left, as -9999 (m0) it is refused.  f1i is f1 with one +Inf pixel at
    APART_INF, inside point 3's box and no other (no excluded pixel there: the clean body).  -> (n0, m0, f1, f1i, xyuvav)"""
    rng = np.random.default_rng(11)
    base = rng.random((96, 96)).astype(np.float32) * 40 + 2
    f0 = base + rng.random((96, 96)).astype(np.float32)
    f1 = np.roll(base, (1, 2), axis=(0, 1)) + rng.random((96, 96)).astype(np.float32)
    xy = np.zeros((4, 6))
    xy[:, 2:4] = [[30, 30], [30, 64], [64, 30], [64, 64]]
    chip = np.ones((15, 15), bool)
    chip.ravel()[rng.choice(225, 30, replace=False)] = False
    n0, m0 = f0.copy(), f0.copy()
    n0[23:38, 23:38][chip] = np.nan
    m0[23:38, 23:38][chip] = -9999.0
    f1i = f1.copy()
    f1i[APART_INF[1], APART_INF[0]] = np.inf
    return n0, m0, np.ascontiguousarray(f1), f1i, xy


FILTERED_OCW, FILTERED_R = (7, 16), 7
FILTERED_KERNELS = (0, 2)               # indices into the CLI kernels: one gradient kernel and the Laplacian


def cli_kernels():
    from mimc3_amd import api
    return api.CLI_KERNELS


def ulp_distance(a, b):
    """Distance in f32 ulps between finite float32 arrays (same shape) -> int64 array."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def surface_distance(got, want, what=""):
    """Asserts that two surfaces have the same finite mask -> (share of finite cells whose bits differ, largest distance in ulps)."""
    fa, fb = np.isfinite(got), np.isfinite(want)
    assert np.array_equal(fa, fb), f"{what}: finite masks differ at {np.argwhere(fa != fb)[:5].tolist()}"
    if not fa.any():
        return 0.0, 0
    d = ulp_distance(got[fa], want[fa])
    return float((d != 0).mean()), int(d.max())
