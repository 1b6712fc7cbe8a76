"""Test infrastructure of the forward-backward consistency check (mimc3_match_ncc_full_fb): fb_chain, the definition of
include/mimc3_hip.h restated on the host over any callable with match_ncc_full_any's signature -- the seed arithmetic, the two-call
chain (one forward call, one backward call over the rows that are searched) and the compose arithmetic -- and the fixture the CPU and GPU
tests share."""
import numpy as np

from full_any_common import encode_nulls, to_float
from full_dn_common import full_dn, to_dn16

FB_OCW, FB_R = 7, 4
FB_OFFSET = np.array([1, -1], np.int32)
FB_TRUE = (3, -2)                       # the fixture's uniform displacement (u, v), i0 -> i1
FB_NOISE_ROW = 84                       # rows >= this of i1 are independent noise


def rint_f32(x):
    """rintf: float32 -> the nearest integer, halves to even (numpy's rint on float32 is that) -> int64"""
    return np.rint(np.asarray(x, np.float32)).astype(np.int64)


def fb_seed(xyuvav, offset, du, dv, ocw, H, W):
    """The rows of the backward search from forward results du, dv float32[P][N] -> (xyuvav' float64[P N][6], shift' int32[P N][2],
    why uint8[P N]: 0 searched, 5 no fit, 6 the chip at m leaves the image)."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    P, N = du.shape
    idx = np.tile(np.arange(N), P)
    du, dv = du.reshape(-1), dv.reshape(-1)
    fit = np.isfinite(du) & np.isfinite(dv)
    with np.errstate(invalid="ignore"):
        small = fit & (np.abs(du) < np.float32(2.0 ** 30)) & (np.abs(dv) < np.float32(2.0 ** 30))
    r = np.zeros((P * N, 2), np.int64)
    r[small, 0] = rint_f32(du[small])
    r[small, 1] = rint_f32(dv[small])
    uv0 = xy[idx, 2:4].astype(np.int32).astype(np.int64)                 # (int) truncates
    m = uv0 + np.asarray(offset, np.int64)[None, :] + r
    inside = (m[:, 0] - ocw >= 0) & (m[:, 0] + ocw < W) & (m[:, 1] - ocw >= 0) & (m[:, 1] + ocw < H)
    why = np.where(~fit, 5, np.where(small & inside, 0, 6)).astype(np.uint8)
    go = why == 0
    xy2 = xy[idx].copy()
    xy2[:, 2:4] = np.where(go[:, None], m, -1).astype(np.float64)
    sh2 = np.where(go[:, None], -r, 0).astype(np.int32)
    return xy2, sh2, why


def fb_compose(du, dv, back, why):
    """fb float32[P][N][4] from the forward du, dv float32[P][N], the backward records float32[P N][8] (rows with why != 0 unused)."""
    P, N = du.shape
    du, dv = du.reshape(-1), dv.reshape(-1)
    fb = np.full((P * N, 4), np.nan, np.float32)
    go = why == 0
    fb[~go, 2] = -why[~go].astype(np.float32)
    fb[go, :3] = back[go, :3]
    fin = go & np.isfinite(back[:, 0]) & np.isfinite(back[:, 1])
    a = du[fin].astype(np.float64) + back[fin, 0].astype(np.float64)
    b = dv[fin].astype(np.float64) + back[fin, 1].astype(np.float64)
    fb[fin, 3] = np.hypot(a, b).astype(np.float32)                       # f64 hypot, rounded once
    return fb.reshape(P, N, 4)


def fb_chain(search, xyuvav, offset, ocw, radius, H, W, npeaks=0, shift=None, mode=0):
    """mimc3_match_ncc_full_fb by its definition: search(xyuvav, offset, ocw, radius, npeaks, shift=, swap=, mode=) -> (record,
    candidates or None) is called once forward and once backward (swap=True, npeaks 0) over the rows that are searched.
    -> (record, candidates or None, fb float32[1 + npeaks][N][4], why uint8[1 + npeaks][N])"""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    N = xy.shape[0]
    out, cand = search(xy, offset, ocw, radius, npeaks, shift=shift, swap=False, mode=mode)
    du = np.concatenate([out[None, :, 0]] + ([cand[:, :, 0]] if npeaks else []))
    dv = np.concatenate([out[None, :, 1]] + ([cand[:, :, 1]] if npeaks else []))
    xy2, sh2, why = fb_seed(xy, offset, du, dv, ocw, H, W)
    back = np.full((xy2.shape[0], 8), np.nan, np.float32)
    go = why == 0
    if go.any():
        back[go] = search(np.ascontiguousarray(xy2[go]), -np.asarray(offset, np.int32), ocw, radius, 0, shift=np.ascontiguousarray(sh2[go]),
                          swap=True, mode=mode)[0]
    return out, cand, fb_compose(du, dv, back, why), why.reshape(1 + npeaks, N)


def oracle_search(i0, i1):
    """The C oracle of the exhaustive search on the integer classes (tests/full_dn_oracle.c) with match_ncc_full_any's signature."""
    def search(xy, offset, ocw, radius, npeaks, shift=None, swap=False, mode=0):
        return full_dn(i0, i1, xy, offset, ocw, radius, npeaks, shift=shift, swap=swap)
    return search


# ---- the fixture ----
def fb_pair(H=160, W=160, seed=41):
    """An 8-bit pair with the uniform displacement FB_TRUE (i1[v][u] = i0[v + 2][u - 3]) and about 1 % null pixels in each image; the rows
    >= FB_NOISE_ROW of i1 are independent noise.  -> (i0, i1) float32"""
    rng = np.random.default_rng(seed)
    n = rng.random((H + 41, W + 41))
    base = (n[:-1, :-1] + n[1:, :-1] + n[:-1, 1:] + n[1:, 1:]) / 4
    base = np.clip(np.rint(1 + 254 * (base - 0.15) / 0.7), 1, 255)
    i0 = base[20:20 + H, 20:20 + W].copy()
    i1 = base[20 - FB_TRUE[1]:20 - FB_TRUE[1] + H, 20 - FB_TRUE[0]:20 - FB_TRUE[0] + W].copy()
    i1[FB_NOISE_ROW:] = rng.integers(1, 256, (H - FB_NOISE_ROW, W))
    for img in (i0, i1):
        img[rng.random((H, W)) < 0.01] = 0
    return np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32)


def fb_points(n=None, ocw=FB_OCW, radius=FB_R, H=160, W=160):
    """The fixture's grid (8 x 7 points) and four more: 56 with its forward peak on the border (shift puts the true displacement on
    su = R), 57 and 58 near the right and the top edge (the landing chip leaves the image), 59 at non-integral coordinates; every search
    centre is FB_OFFSET + shift.  -> (xyuvav float64[60][6], shift int32[60][2]); n: the first n of them"""
    us, vs = np.linspace(ocw + 7, W - 13 - ocw, 8).astype(int), np.linspace(ocw + 7, H - 7 - ocw, 7).astype(int)
    pts = [(u, v) for v in vs for u in us] + [(W // 2 - 20, H // 2 - 40), (W - 2 - ocw, ocw + 23), (W // 2, ocw + 1), (100.75, 50.25)]
    xy = np.zeros((len(pts), 6))
    xy[:, 2:4] = pts
    xy[:, 0] = 1000.0 + 15.0 * xy[:, 2]
    xy[:, 1] = 5000.0 - 15.0 * xy[:, 3]
    shift = np.tile(np.array([[1, 0]], np.int32), (len(pts), 1))         # true - offset - shift = (1, -1): an interior cell
    shift[56] = (FB_TRUE[0] - FB_OFFSET[0] - radius, 0)                  # ... = (R, -1): su = R
    shift[3] = (2, -2)
    shift[10] = (0, 1)
    if n is not None:
        xy, shift = xy[:n], shift[:n]
    return np.ascontiguousarray(xy), np.ascontiguousarray(shift)


def fb_areas(xy, ocw=FB_OCW, radius=FB_R):
    """(shifted, noise): the points whose forward box lies in the rows i1 took from i0, and those whose box lies in the noise rows"""
    v = xy[:, 3].astype(int) + FB_OFFSET[1]
    reach = ocw + radius + 2
    return v + reach < FB_NOISE_ROW, v - reach >= FB_NOISE_ROW


def class_pair(kind):
    """The fixture's pair in one pixel class -> (i0, i1, the path name match_ncc_full_any reports in mode 0)"""
    i0, i1 = fb_pair()
    if kind == "u8":
        return i0, i1, "u8_mfma_full"
    if kind == "dn12":
        return np.ascontiguousarray(i0 * 16), np.ascontiguousarray(i1 * 16), "u16_full"
    if kind == "dn16":
        return to_dn16(i0, 51), to_dn16(i1, 52), "f32i_full"
    assert kind == "float"
    f0, f1 = encode_nulls(to_float(i0, 53), to_float(i1, 54), "m9999_nan")     # -9999 nulls in image 0, NaN nulls in image 1
    return f0, f1, "f32g_full"
