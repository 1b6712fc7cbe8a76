"""Test infrastructure: the coarse-to-fine exhaustive search on any f32 pair (mimc3_match_ncc_pyramid_any, include/mimc3_hip.h) restated on
the CPU -- the float reduction in numpy (float64 additions in the stated order, one rounding to float32), every coarser level's search
through full_any_common.full_any's surface in the reference's summation order (order 0), the first-wins arg-max over its finite cells in
k order, the chip and border rules of pyramid_oracle._inside, and level 0 through full_any with its candidates.

The device sums in an order of its own, so a device cell may sit 1 f32 ulp from the oracle's (the bound of mimc3_match_ncc_full_any):
where the oracle's best cell of a coarser level does not lead every other finite cell by more than 2 ulps, the arg-max is not determined
by the definition, and the point is UNDECIDED -- pyramid_search_any reports those points, and at most UNDECIDED_CAP of a case's points
may be so."""
import numpy as np

from full_any_common import full_any, ulp_distance
from pyramid_dn_oracle import surface_peaks
from pyramid_oracle import _inside

MIN_DN = 1e-10
UNDECIDED_CAP = 0.02


def reduce2_any(img):
    """One float level: pixel = float32(S / n), S the float64 sum of the block's included pixels (float64(p) >= MIN_DN) added in the order
    (2y, 2x), (2y, 2x + 1), (2y + 1, 2x), (2y + 1, 2x + 1) and n their number, 0 when n = 0; an odd last row or column is dropped."""
    a = np.asarray(img, np.float32)
    H, W = a.shape[0] >> 1, a.shape[1] >> 1
    S = np.zeros((H, W), np.float64)
    n = np.zeros((H, W), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            d = a[dy:2 * H:2, dx:2 * W:2].astype(np.float64)
            inc = d >= MIN_DN                                   # (False for NaN)
            S = S + np.where(inc, d, 0.0)
            n += inc
        out = np.where(n > 0, S / np.maximum(n, 1), 0.0).astype(np.float32)
    return np.ascontiguousarray(out)


def pyramid_any(img, levels):
    """[level 0 (the image), level 1, ...]"""
    out = [np.ascontiguousarray(img, np.float32)]
    for _ in range(1, levels):
        out.append(reduce2_any(out[-1]))
    return out


def undecided_peaks(surf, margin=2):
    """bool[N]: the largest finite cell does not exceed every other finite cell by more than `margin` f32 ulps."""
    fin = np.isfinite(surf)
    v = np.sort(np.where(fin, surf, -np.inf), axis=1)
    two = fin.sum(axis=1) >= 2
    best, second = v[:, -1], v[:, -2]
    out = np.zeros(surf.shape[0], bool)
    out[two] = ulp_distance(best[two], second[two]) <= margin
    return out


def level_peaks_any(i0l, i1l, pos, d, ocw, R, swap=False):
    """The arg-max k of the exhaustive search on one level at pos with offset 0 and shift d (-1 where there is none), and where it is
    undecided -> (int64[N], bool[N])"""
    H, W = i0l.shape
    ok = _inside(pos, d, ocw, R, H, W)
    peak = np.full(pos.shape[0], -1, np.int64)
    und = np.zeros(pos.shape[0], bool)
    if ok.any():
        xy = np.zeros((int(ok.sum()), 6))
        xy[:, 2:4] = pos[ok]
        surf = full_any(i0l, i1l, xy, (0, 0), ocw, R, 0, shift=d[ok].astype(np.int32), swap=swap, order=0)[2]
        peak[ok] = surface_peaks(surf)
        und[ok] = undecided_peaks(surf)
    return peak, und


def pyramid_search_any(i0, i1, xyuvav, offset, ocw, radius, levels, npeaks=0, shift=None, swap=False):
    """-> (float32[N][8] record, float32[npeaks][N][3] candidates or None, int32[N][2] shift_out, bool[N] undecided on some coarser
    level), the definition step by step."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    off = np.asarray(offset, np.int64).reshape(1, 2)
    D = off + (np.zeros((n, 2), np.int64) if shift is None else np.asarray(shift, np.int64))
    uv0 = xy[:, 2:4].astype(np.int64)                          # (int) truncation
    L = int(levels)
    d = D if L == 1 else (D + (1 << (L - 2))) >> (L - 1)       # floor((D + 2^(L-2)) / 2^(L-1))
    p0, p1 = pyramid_any(i0, L), pyramid_any(i1, L)
    S = 2 * radius + 1
    undecided = np.zeros(n, bool)
    for lv in range(L - 1, 0, -1):
        pk, und = level_peaks_any(p0[lv], p1[lv], uv0 >> lv, d, ocw, radius, swap)
        undecided |= und
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - radius, pk % S - radius], axis=1), 0)
        d = 2 * (d + s)
    shift_out = (d - off).astype(np.int32)
    rec, cand = full_any(i0, i1, xy, offset, ocw, radius, npeaks, shift=shift_out, swap=swap, order=0)[:2]
    H, W = np.asarray(i0).shape
    out = ~_inside(uv0, d, ocw, radius, H, W)
    rec[out] = np.nan
    if cand is not None:
        cand[:, out] = np.nan
    return rec, cand, shift_out, undecided


# ---- fixtures the CPU and GPU tests share ----
def hand_blocks():
    """A 7 x 29 image (odd: the last row and column are dropped) whose first two rows hold 14 hand-made blocks -> (image, the 14 level
    pixels as float64 means to be rounded to float32).  Every n from 0 to 4; NaN, -9999, -0.0, 1e-11 (below MIN_DN), 1e-9 (above) and +Inf
    members; an all-NaN block."""
    nan, inf = np.nan, np.inf
    blocks = [
        ((1.5, 2.25, 3.125, 4.0625), (1.5 + 2.25 + 3.125 + 4.0625) / 4),          # n = 4
        ((1.5, nan, 3.125, 4.0625), ((1.5 + 3.125) + 4.0625) / 3),                # n = 3, a NaN
        ((-9999.0, 0.1, 0.7, -9999.0), (np.float64(np.float32(0.1)) + np.float64(np.float32(0.7))) / 2),       # n = 2
        ((0.0, 0.0, 0.0, 0.3), np.float64(np.float32(0.3))),                      # n = 1
        ((0.0, 0.0, 0.0, 0.0), 0.0),                                              # n = 0
        ((nan, nan, nan, nan), 0.0),                                              # all NaN: the canonical null
        ((-0.0, 5.0, -0.0, 7.0), 6.0),                                            # -0.0 is excluded
        ((1e-11, 1e-11, 1e-11, 2.0), 2.0),                                        # below MIN_DN: excluded
        ((1e-9, 0.0, 0.0, 0.0), np.float64(np.float32(1e-9))),                    # above MIN_DN: included
        ((1e-9, 1e-11, nan, -9999.0), np.float64(np.float32(1e-9))),
        ((inf, 1.0, 2.0, 3.0), inf),                                              # an included +Inf goes through
        ((inf, nan, 0.0, -1.0), inf),
        ((-inf, 3.0, nan, 0.0), 3.0),                                             # -Inf is a negative: excluded
        ((16777216.0, 1.0, 1.0, 1.0), (16777216.0 + 3.0) / 4),                    # the f64 sum keeps what an f32 sum would lose
    ]
    img = np.random.default_rng(3).random((7, 29)).astype(np.float32) + np.float32(0.5)
    want = np.empty(len(blocks), np.float64)
    for k, (b, w) in enumerate(blocks):
        img[0:2, 2 * k:2 * k + 2] = np.array(b, np.float32).reshape(2, 2)
        want[k] = w
    return np.ascontiguousarray(img), want


def upsampled_pair(bits, seed, small=(72, 80), motion=(3, -2), null_frac=0.004):
    """A 4 x-upsampled integer pair: 8-, 12- or 16-bit small images (the second one the first moved by whole small-scale pixels `motion`,
    with noise), np.kron with a 4 x 4 block of ones, then single-pixel nulls punched in at random.  Every 2 x 2 block of levels 0 and 1
    holds equal included pixels, so the rounded integer mean and the float mean agree: float levels 1 and 2 are the integer levels.
    -> (i0, i1, xyuvav of 20 points)"""
    from full_dn_common import to_dn16
    from mimc3_amd import synth
    from pyramid_dn_oracle import dn12_low
    s0, s1 = synth.make_pair(small[0], small[1], motion, seed, noise_dn=2, pad=16, sigma=1.0)
    if bits == 12:
        s0, s1 = dn12_low(s0, seed + 1), dn12_low(s1, seed + 2)
    elif bits == 16:
        s0, s1 = to_dn16(s0, seed + 1), to_dn16(s1, seed + 2)
    else:
        assert bits == 8
    rng = np.random.default_rng(seed + 3)
    out = []
    for s in (s0, s1):
        a = np.kron(s, np.ones((4, 4), np.float32)).astype(np.float32)
        a[rng.random(a.shape) < null_frac] = 0
        out.append(np.ascontiguousarray(a))
    xy = synth.make_grid(5, 4, 60, 56, 50, 58, 700.0, angle_deg=40.0)
    return out[0], out[1], xy


def float_pyr_case(ocw, null_frac, seed, levels, encoding="zero"):
    """pyramid_dn_oracle.case's pair and grid (odd sizes, a coarsest level that just holds a chip, a motion the prior misses) as
    non-integral floats with the nulls in `encoding` -> (case, f0, f1)"""
    from full_any_common import encode_nulls, to_float
    from pyramid_dn_oracle import case
    c = case(ocw, null_frac, seed, levels)
    f0, f1 = encode_nulls(to_float(c.i0, 3000 + seed), to_float(c.i1, 4000 + seed), encoding)
    return c, f0, f1


def big_float_case():
    """pyramid_oracle.big_case, the pair moved by (+70, -45) px, as non-integral floats with a few null discs, the nulls NaN in image 0
    -> (f0, f1, xyuvav)"""
    from full_any_common import encode_nulls, to_float
    from mimc3_amd import synth
    from pyramid_oracle import big_case
    b0, b1, g = big_case()
    b0, b1 = b0.copy(), b1.copy()
    rng = np.random.default_rng(63)
    synth._blobs(b0, 0.01, rng)
    synth._blobs(b1, 0.01, rng)
    f0, f1 = encode_nulls(to_float(b0, 61), to_float(b1, 62), "nan_zero")
    assert np.isnan(f0).any() and (f1 == 0).any()
    return f0, f1, g


# the cases of the GPU test against this oracle (tests/test_pyramid_any.py), whose undecided share tests/test_pyramid_any_oracle.py caps
ORACLE_R, ORACLE_LEVELS = 6, 3
ORACLE_CASES = [(kind, ocw) for kind in ("zero", "m9999_nan", "wide") for ocw in (7, 16)]


def oracle_case(kind, ocw):
    """-> (case, f0, f1, a-priori shift): float_case with the encoding `kind`, or wide_case"""
    from full_any_common import float_case, wide_case
    if kind == "wide":
        return wide_case(ocw, 0.03, ORACLE_R)
    return float_case(ocw, 0.03, ORACLE_R, kind)
