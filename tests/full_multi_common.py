"""Test infrastructure: the test-side oracle of the exhaustive search with candidates (tests/full_multi_oracle.c), compiled on first use
into tests/_build with the flags tests/full_search_common.py uses, a brute-force Python restatement of the local-maximum rule and
its rank for small cases, the oracle's post-matcher chain over stacked candidates, and the fixtures the CPU and GPU tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from full_search_common import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "full_multi_oracle.c")
LIB = os.path.join(HERE, "_build", "libfull_multi_oracle.so")
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
        lib.full_multi.argtypes = [_f32p, _f32p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.c_int, _f32p, _f32p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        lib.full_multi.restype = C.c_int
        _lib = lib
    return _lib


def full_multi(i0, i1, xyuvav, offset, ocw, radius, npeaks, shift=None, swap=False, with_counts=False, lmcap=0, nthreads=0):
    """The exhaustive search with candidates on the CPU -> (float32[N][8] record, float32[npeaks][N][3] candidates), then, if asked
    for, the number of local maxima per point (with_counts) and the first lmcap ranked local maxima's k per point, -1 behind the last."""
    i0 = np.ascontiguousarray(i0, np.float32)
    i1 = np.ascontiguousarray(i1, np.float32)
    xy = np.ascontiguousarray(xyuvav, np.float64)
    H, W = i0.shape
    n = xy.shape[0]
    out = np.empty((n, 8), np.float32)
    cand = np.empty((npeaks, n, 3), np.float32)
    nlm = np.empty(n, np.int32)
    lmk = np.empty((n, max(lmcap, 1)), np.int32)
    sh = None if shift is None else np.ascontiguousarray(shift, np.int32)
    rc = _load().full_multi(i0, i1, H, W, xy, n, int(offset[0]), int(offset[1]), None if sh is None else sh.ctypes.data, ocw, radius,
                            npeaks, 1 if swap else 0, out, cand.reshape(-1), nlm.ctypes.data, lmk.ctypes.data if lmcap else None, lmcap, nthreads)
    if rc != 0:
        raise ValueError(f"full_multi rc={rc}")
    res = (out, cand)
    if with_counts:
        res += (nlm,)
    if lmcap:
        res += (lmk,)
    return res


def filled_fraction(out, cand):
    """Of the points with a non-negative status in the record, the fraction whose every candidate slot holds a peak."""
    ok = out[:, 2] >= -1
    return float((cand[:, ok, 2] >= -1).all(axis=0).mean()) if ok.any() else 0.0


# ---- fixtures the CPU and GPU tests share ----
def parity_case(ocw, null_frac, radius, dimx=6, dimy=5):
    """A make_small pair and grid as tests/test_full_search.py's, but on a nearly white texture (sigma 0.3 px): the local maxima of an
    NCC surface are about as dense as its texture is rough -- the default sigma of 2 px leaves a 31 x 31 surface some 5 of them, sigma 0.3
    about one per 9 cells, so that 8 slots fill at R = 7 too (tests/test_full_multi_oracle.py asserts it).  -> (case, a-priori shift)"""
    from mimc3_amd import api, synth
    c = synth.make_small(seed=7100 + ocw + int(100 * null_frac) + radius, shift=(3, -2), angle_deg=40.0, ocw=ocw, speed=700.0,
                         h=2 * ocw + 200, w=2 * ocw + 210, dimx=dimx, dimy=dimy, noise_dn=2, null_frac=null_frac, offset=(1, -1), sigma=0.3)
    return c, api.prior_shift(c.xyuvav, c.dt, c.mpp)


STATUS_R = 5


def status_case():
    """tests/test_full_search.py's edge pair on a rough texture, for ocw 7 and R = STATUS_R: point 0's box is > 80 % null (-3), point 1's
    chip is flat (-2: no finite cell), point 2's true offset (+5, 0) is a border cell of the search (-4) while its interior keeps the
    local maxima of a rough surface, and points 3-5 overhang the image edge.  -> (i0, i1, xyuvav)"""
    from mimc3_amd import synth
    H = W = 128
    i0 = synth.texture(H, W, 3, sigma=0.5)
    i1 = np.roll(i0, (0, 5), axis=(0, 1)).copy()
    i1[10:70, 10:70] = 0
    i0[80 - 7:80 + 8, 40 - 7:40 + 8] = 9
    xy = np.zeros((6, 6))
    xy[:, 2:4] = [[40, 40], [40, 80], [90, 90], [7, 60], [120, 120], [60, 7]]
    return i0, i1, xy


def periodic_pair(pu, pv, plateau, seed=9):
    """An exactly periodic 8-bit pair without nulls, 200 x 200, and six grid points.  B has period pu x pv px (values 1..120).
    plateau False: i0 = i1 = B -- offsets a period apart have identical integer sums, i.e. bit-equal NCC.
    plateau True:  i0 = B, i1 = B + (B moved one row down); with a chip and a box of whole periods, sum a b at (su, sv) is
    C(s) + C(s - e_v) for the periodic autocorrelation C = C(-s): equal at sv = 0 and sv = 1 (mod pv), the flat top."""
    rng = np.random.default_rng(seed)
    tile = rng.integers(1, 121, (pv, pu))
    B = np.tile(tile, (200 // pv + 2, 200 // pu + 2))[:200, :200].astype(np.float32)
    i1 = B + np.roll(np.tile(tile, (200 // pv + 2, 200 // pu + 2)), 1, axis=0)[:200, :200].astype(np.float32) if plateau else B.copy()
    xy = np.zeros((6, 6))
    xy[:, 2:4] = [[80, 80], [81, 83], [100, 90], [97, 104], [110, 85], [92, 111]]
    return B, np.ascontiguousarray(i1, np.float32), xy


DECOY_OCW, DECOY_R, DECOY_TRUE = 7, 15, (3, -2)


def decoy_case():
    """A 10 x 9 grid on a rough pair (sigma 0.6 px, +-2 DN noise) displaced by DECOY_TRUE, with a decoy at four isolated grid points:
    in i1 the chip-sized block at the point's true position gets +-6 DN of extra noise, and a clean copy of that block is pasted
    (-12, +9) px away, inside +-R = 15.  The copy correlates perfectly, the damaged truth a little less: the global peak is the decoy,
    the truth the second local maximum.  -> (case with the doctored i1, a-priori shift, the four points' indices)"""
    from mimc3_amd import api, synth
    import dataclasses
    ocw = DECOY_OCW
    c = synth.make_small(seed=41, shift=DECOY_TRUE, angle_deg=30.0, ocw=ocw, speed=900.0, h=420, w=440, dimx=10, dimy=9, noise_dn=2,
                         margin=70, sigma=0.6)
    rng = np.random.default_rng(41)
    i1 = c.i1.copy()
    pts = [2 * 10 + 2, 2 * 10 + 7, 6 * 10 + 3, 6 * 10 + 7]
    for g in pts:
        tu, tv = int(c.xyuvav[g, 2]) + DECOY_TRUE[0], int(c.xyuvav[g, 3]) + DECOY_TRUE[1]
        clean = c.i1[tv - ocw:tv + ocw + 1, tu - ocw:tu + ocw + 1].copy()
        i1[tv - ocw:tv + ocw + 1, tu - ocw:tu + ocw + 1] = np.clip(clean + rng.integers(-6, 7, clean.shape), 1, 255)
        i1[tv + 9 - ocw:tv + 9 + ocw + 1, tu - 12 - ocw:tu - 12 + ocw + 1] = clean
    c = dataclasses.replace(c, i1=np.ascontiguousarray(i1, np.float32))
    return c, api.prior_shift(c.xyuvav, c.dt, c.mpp), pts


def decoy_errors(field, pts):
    """|displacement - truth| in px of a [5][N] post-processed field: (at the decoy points, the largest elsewhere)"""
    err = np.hypot(field[0] - DECOY_TRUE[0], field[1] - DECOY_TRUE[1])
    return err[pts], float(np.nanmax(np.delete(err, pts)))


# ---- brute force, small cases: the surface in numpy (int64 sums, the f64 formula), the rule and the rank as the header words them ----
def surface_py(i0, i1, u0, v0, cu, cv, ocw, R):
    """val[x][y], x = su + R, y = sv + R, or None at a point the validity rule (> 0.8 nulls) refuses"""
    H, W = i0.shape
    cw, S = 2 * ocw + 1, 2 * R + 1
    a = i0[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1].astype(np.int64)
    h = R + ocw
    box = np.zeros((2 * h + 1, 2 * h + 1), np.int64)
    for y in range(2 * h + 1):
        for x in range(2 * h + 1):
            pu, pv = cu - h + x, cv - h + y
            if 0 <= pu < W and 0 <= pv < H:
                box[y, x] = int(i1[pv, pu])
    if np.float32((a == 0).sum()) / np.float32(cw * cw) > np.float32(0.8) or \
            np.float32((box == 0).sum()) / np.float32(box.size) > np.float32(0.8):
        return None
    val = np.empty((S, S), np.float32)
    with np.errstate(all="ignore"):
        for x in range(S):
            for y in range(S):
                b = box[y:y + cw, x:x + cw]
                m = (a != 0) & (b != 0)
                n, sx, sy = int(m.sum()), int(a[m].sum()), int(b[m].sum())
                sxx, syy, sxy = int((a[m] ** 2).sum()), int((b[m] ** 2).sum()), int((a[m] * b[m]).sum())
                dn, dsx, dsy = np.float64(n), np.float64(sx), np.float64(sy)
                val[x, y] = np.float32((dn * np.float64(sxy) - dsx * dsy) /
                                       np.sqrt((dn * np.float64(sxx) - dsx * dsx) * (dn * np.float64(syy) - dsy * dsy)))
    return val


def ranked_local_maxima_py(val):
    """the k of every local maximum of val[x][y], ranked by NCC descending, ties by ascending k"""
    S = val.shape[0]
    R = S // 2
    found = []
    for su in range(-R + 1, R):
        for sv in range(-R + 1, R):
            v = val[su + R, sv + R]
            k = (su + R) * S + (sv + R)
            if not np.isfinite(v):
                continue
            good = True
            for du in (-1, 0, 1):
                for dv in (-1, 0, 1):
                    if du == 0 and dv == 0:
                        continue
                    t = val[su + du + R, sv + dv + R]
                    kt = (su + du + R) * S + (sv + dv + R)
                    if not (not np.isfinite(t) or v > t or (v == t and k < kt)):
                        good = False
            if good:
                found.append((-float(v), k))
    return [k for _, k in sorted(found)]


# ---- the oracle's post-matcher chain over candidates dp [ndp][N][3]: the oracle's stages (oracle/oracle.py: cluster_candidates, get_dpf0,
#      get_dpf1, get_ruv_neighbor, qm) chained as mimc2_postprocess chains them -- postprocess_edge_common.oracle_chain, imported as it is
def oracle_postprocess(oracle, dp, xyuvav, dimx, dimy, mps, dt, mpp):
    """-> planes float32[5][N] (du, dv, their variances, quality; px units), what Context.mimc2_postprocess returns as [5][dimy][dimx]"""
    from postprocess_edge_common import oracle_chain
    return oracle_chain(oracle, np.ascontiguousarray(dp, np.float32), xyuvav, dimx, dimy, mps, dt=dt, mpp=mpp)[0]
