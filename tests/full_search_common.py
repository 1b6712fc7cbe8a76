"""Test infrastructure: the test-side oracle of the exhaustive search (tests/full_search_oracle.c), compiled on first use into
tests/_build with the repository oracle's flags, and a comparison helper for its [N][8] records (bit for bit but the SNR, within 1 f32 ulp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "full_search_oracle.c")
LIB = os.path.join(HERE, "_build", "libfull_search_oracle.so")
FLAGS = ["-O3", "-fno-tree-slp-vectorize", "-fopenmp", "-ffp-contract=off", "-fPIC", "-shared", "-std=gnu11", "-Wall"]
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
        lib.full_search.argtypes = [_f32p, _f32p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, _f32p, C.c_void_p, C.c_int]
        lib.full_search.restype = C.c_int
        _lib = lib
    return _lib


def full_search(i0, i1, xyuvav, offset, ocw, radius, shift=None, swap=False, with_peak=False, nthreads=0):
    """The exhaustive search on the CPU -> float32[N][8] (and the arg-max k per point, -1 without one, if with_peak)."""
    i0 = np.ascontiguousarray(i0, np.float32)
    i1 = np.ascontiguousarray(i1, np.float32)
    xy = np.ascontiguousarray(xyuvav, np.float64)
    H, W = i0.shape
    n = xy.shape[0]
    out = np.empty((n, 8), np.float32)
    peak = np.empty(n, np.int32)
    sh = None if shift is None else np.ascontiguousarray(shift, np.int32)
    rc = _load().full_search(i0, i1, H, W, xy, n, int(offset[0]), int(offset[1]), None if sh is None else sh.ctypes.data, ocw, radius,
                             1 if swap else 0, out, peak.ctypes.data, nthreads)
    if rc != 0:
        raise ValueError(f"full_search rc={rc}")
    return (out, peak) if with_peak else out


def assert_records_match(got, want, what=""):
    """Columns 0-3 and 5-7 bit for bit (NaN == NaN): the fit's value and Hessian take the same float / double operations in the same
    order on both sides.  Column 4 (SNR) within 1 f32 ulp of the larger magnitude: its f64 sum of squares runs in another order."""
    from conftest import assert_bits_equal
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    assert_bits_equal(got[:, :4], want[:, :4], what + " (du, dv, ncc_peak, ncc_fit)")
    assert_bits_equal(got[:, 5:], want[:, 5:], what + " (h_uu, h_uv, h_vv)")
    a, b = got[:, 4], want[:, 4]
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN masks of the SNR differ at {np.argwhere(na != nb)[:5].tolist()}"
    a = np.where(na, 0, a); b = np.where(nb, 0, b)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    bad = np.argwhere(np.abs(a.astype(np.float64) - b.astype(np.float64)) > ulp)
    assert bad.size == 0, f"{what}: {len(bad)} SNR values beyond 1 f32 ulp, first {bad[:3].ravel().tolist()} {a[bad[0]]!r} vs {b[bad[0]]!r}"
