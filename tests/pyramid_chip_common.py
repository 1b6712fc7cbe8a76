"""Test infrastructure: the fixtures of the coarse-to-fine exhaustive search at any chip size (mimc3_match_ncc_pyramid_chip) that the CPU
and GPU tests share.  Nothing here is a new definition: the pairs are pyramid_dn_oracle.case / as_class and
pyramid_any_oracle.float_pyr_case, the expected results come from pyramid_search_dn / pyramid_search_any (their C oracles take any
chip size), and what is added is the call list of the parity test and the classification of a coarser level's points into what the
two forms of a matrix-core kernel do with them."""
import functools

import numpy as np

from pyramid_dn_oracle import as_class, case, pyramid_dn, pyramid_search_dn
from pyramid_oracle import _inside

PAD = 256                                   # the planes' zero border
SIX = (7, 15, 16, 30, 32, 40)
CLASSES = ("u8", "u16", "f32")              # 8-bit, 12-bit DN with low-order entropy, full-entropy 16-bit DN
CLASS_INDEX = {"u8": 0, "u16": 1, "f32": 2, "float": 3}
PATH_NAME = {6: "u8_mfma_full", 7: "u16_full", 8: "f32i_full", 9: "f32g_full", 11: "f32g_chip", 12: "u8_mfma_chip", 13: "u16_mfma_chip"}
R = 5                                       # the radius of every case but the R-15 ones
PARITY_OCW = (10, 24, 25, 45, 57)           # both sides of the two KCW thresholds (24 | 25, 56 | 57)
# What one (class, ocw) parity test runs: (levels, null fraction, npeaks, swap), the full product of L 2 and 3, null fractions 0 and 0.15,
# npeaks 0 and 4 and both directions -- sixteen calls on four pairs
PARITY_COMBOS = tuple((L, nf, npk, sw) for L in (2, 3) for nf in (0.0, 0.15) for npk in (0, 4) for sw in (False, True))
# ... and the one R-15 call per matrix-core kernel, at the largest chip
R15_CALL = (80, 15, 2, 0.15, 4, False)      # ocw, R, levels, null fraction, npeaks, swap


def table_path(cls, ocw, mode):
    """The issue's level / kernel table, restated: last_path of mimc3_match_ncc_pyramid_chip, 0 outside it."""
    if not 1 <= ocw <= 80 or mode not in (0, 1) or cls not in CLASS_INDEX:
        return 0
    six = mode == 0 and ocw in SIX
    return {"u8": 6 if six else 12, "u16": 13, "f32": 8 if six else 11, "float": 9 if six else 11}[cls]


@functools.lru_cache(maxsize=None)
def pair(cls, ocw, null_frac, levels):
    """-> (case, i0, i1, a-priori shift) of one parity call: pyramid_dn_oracle.case at (2 ocw + 1) 2^(L-1) + 45 px, in the class"""
    from mimc3_amd import api
    c = case(ocw, null_frac, 9800 + ocw + int(100 * null_frac) + levels, levels)
    i0, i1 = (c.i0, c.i1) if cls == "u8" else as_class(cls, c, ocw)
    return c, i0, i1, api.prior_shift(c.xyuvav, c.dt, c.mpp)


def parity_calls(cls, ocw):
    """-> [(what, case, i0, i1, offset, shift, ocw, R, levels, npeaks, swap)] of one parity test"""
    combos = [(ocw, R) + k for k in PARITY_COMBOS] if ocw != 80 else [R15_CALL]
    out = []
    for o, r, levels, nf, npeaks, swap in combos:
        c, i0, i1, shift = pair(cls, o, nf, levels)
        off, sh = (-c.offset, -shift) if swap else (c.offset, shift)
        out.append((f"{cls} ocw {o} R {r} L {levels} nulls {nf} npeaks {npeaks} swap {swap}", c, i0, i1, off, sh, o, r, levels, npeaks, swap))
    return out


@functools.lru_cache(maxsize=None)
def _expected(cls, ocw, idx):
    what, c, i0, i1, off, sh, o, r, levels, npeaks, swap = parity_calls(cls, ocw)[idx]
    return pyramid_search_dn(i0, i1, c.xyuvav, off, o, r, levels, npeaks, shift=sh, swap=swap, with_peaks=True)


def expected(cls, ocw, idx):
    """pyramid_search_dn of parity call `idx`, computed once: (record, candidates, shift_out, peaks per coarser level, coarsest first).
    The arrays are shared: do not write to them."""
    return _expected(cls, ocw, idx)


def pick(cls, ocw, levels, npeaks):
    """-> [(idx, call)] of the parity calls of (cls, ocw) with that many levels and candidates"""
    return [(i, k) for i, k in enumerate(parity_calls(cls, ocw)) if k[8] == levels and k[9] == npeaks]


def kcw_class(ocw):
    """K chunks per chip row of the matrix-core kernels: 1 (ocw <= 24), 2 (<= 56), 3"""
    return 1 if ocw <= 24 else 2 if ocw <= 56 else 3


def level_displacements(xyuvav, offset, shift, R, levels, peaks):
    """The displacement d_l the search of each coarser level runs around, from the oracle's peaks -> [d_{L-1}, ..., d_1] (int64 [N][2])"""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    off = np.asarray(offset, np.int64).reshape(1, 2)
    D = off + (np.zeros((xy.shape[0], 2), np.int64) if shift is None else np.asarray(shift, np.int64))
    d = D if levels == 1 else (D + (1 << (levels - 2))) >> (levels - 1)
    S = 2 * R + 1
    out = []
    for pk in peaks:
        out.append(d)
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - R, pk % S - R], axis=1), 0)
        d = 2 * (d + s)
    return out


def launch_kinds(chip_img, win_img, pos, d, ocw, R, peak):
    """What the two forms of a matrix-core kernel do with each point of one coarser-level launch, on the oracle's level images ->
    list of "clean" (the clean form finishes it with a peak), "masked" (the masked form does: a null in its chip or its search box, the
    zero border included), "none" (no arg-max: the chip leaves the level, the box leaves the border, -3, or no finite cell) or "other"
    (a peak the clean form stores with status -4 is still "clean": the kinds are about which form writes the cell)."""
    H, W = chip_img.shape
    cp = np.pad(np.asarray(chip_img), PAD)
    wp = np.pad(np.asarray(win_img), PAD)
    ok = _inside(pos, d, ocw, R, H, W)
    out = []
    for g in range(pos.shape[0]):
        if not ok[g] or peak[g] < 0:
            out.append("none")
            continue
        u, v = pos[g] + PAD
        cu, cv = pos[g] + d[g] + PAD
        h = ocw + R
        nulls = (cp[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1] == 0).sum() + (wp[cv - h:cv + h + 1, cu - h:cu + h + 1] == 0).sum()
        out.append("masked" if nulls else "clean")
    return out


def call_kinds(call, exp):
    """The kinds of every coarser-level launch of one parity call -> [(level, kinds)]"""
    what, c, i0, i1, off, sh, ocw, r, levels, npeaks, swap = call
    peaks = exp[3]
    p0, p1 = pyramid_dn(i0, levels), pyramid_dn(i1, levels)
    ds = level_displacements(c.xyuvav, off, sh, r, levels, peaks)
    uv0 = np.ascontiguousarray(c.xyuvav, np.float64)[:, 2:4].astype(np.int64)
    out = []
    for k, lv in enumerate(range(levels - 1, 0, -1)):
        chip, win = (p1[lv], p0[lv]) if swap else (p0[lv], p1[lv])
        out.append((lv, launch_kinds(chip, win, uv0 >> lv, ds[k], ocw, r, peaks[k])))
    return out


# ---- the stale-peak fixture: one pair, two calls on the same point indices -----------------------------------------------------------
STALE = dict(ocw=10, R=5, levels=2, H=221, W=235)
STALE_NULL = (slice(20, 70), slice(150, 200))       # rows, columns of i0: all null -- a level-1 chip at (87, 22) lies in it: -3
STALE_FLAT = (slice(150, 200), slice(30, 80))       # ... all one value -- a level-1 chip at (27, 87) lies in it: no finite cell, -2
STALE_POINTS = {0: "chip", 1: "border", 2: "minus3", 3: "minus2"}


@functools.lru_cache(maxsize=None)
def stale_case(cls):
    """-> (i0, i1, xy of the first call, xy of the second, shift of the second).  The first call's 30 points all lie in textured ground;
    the second moves four of them (the same indices) to where level 1 gives no arg-max, one per reason:
      0  u0 = ocw: the chip is inside level 0 but leaves level 1 (u0 >> 1 < ocw)
      1  a shift of W + 601 px: the box lies beyond the zero border on both levels (the all-NaN record)
      2  the chip in an all-null block of i0: status -3 from the masked form
      3  the chip in a flat block of i0: every cell 0 / 0, no finite cell, status -2 (an all-NULL window cannot give -2 on a coarser
         level: a null there is the pixel 0 in every level set, which the validity rule counts, so it gives -3 like point 2)"""
    from full_any_common import to_float
    from mimc3_amd import synth
    s = STALE
    c = synth.make_small(seed=9907, shift=(3, -2), angle_deg=40.0, ocw=s["ocw"], speed=700.0, h=s["H"], w=s["W"], dimx=6, dimy=5,
                         noise_dn=2, null_frac=0.0, offset=(0, 0), sigma=3.0, margin=85)
    b0, b1 = c.i0.copy(), c.i1.copy()
    b0[STALE_NULL] = 0
    if cls == "u8":
        i0, i1 = b0, b1
    elif cls == "float":
        i0, i1 = to_float(b0, 3907), to_float(b1, 4907)
    else:
        class _C:
            pass
        k = _C()
        k.i0, k.i1 = b0, b1
        i0, i1 = as_class(cls, k, 7)
    i0 = i0.copy()
    i0[STALE_FLAT] = {"u8": 64, "u16": 1024, "f32": 1024, "float": 0.5}[cls]      # (a power of two: every f32 product with it is exact)
    i0, i1 = np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32)
    xy1 = np.ascontiguousarray(c.xyuvav, np.float64)
    xy2 = xy1.copy()
    xy2[0, 2:4] = (s["ocw"], 100)
    xy2[2, 2:4] = (175, 45)
    xy2[3, 2:4] = (55, 175)
    shift2 = np.zeros((xy2.shape[0], 2), np.int32)
    shift2[1] = (s["W"] + 601, 0)                   # (even: d_0 = 2 d_1 is the shift itself)
    return i0, i1, xy1, xy2, shift2


# ---- the judge, and the float case against the reference-order oracle ----------------------------------------------------------------
def compare(got, want, what):
    """(record, candidates, shift_out) of the entry against the oracle's: shift_out exactly, the record as assert_records_match compares
    it -- bit for bit but the SNR, whose f64 sum of squares the oracle adds in another order: within 1 f32 ulp, the oracle's own
    error -- and the candidates bit for bit."""
    from conftest import assert_bits_equal
    from full_search_common import assert_records_match
    np.testing.assert_array_equal(got[2], want[2], what + ": shift_out")
    assert_records_match(got[0], want[0], what)
    if want[1] is None:
        assert got[1] is None, what
    else:
        assert_bits_equal(got[1], want[1], what + ": candidates")


FLOAT_OCW = (10, 33)                        # one band of the float kernel's chip walk, and several (KCW does not exist there)


@functools.lru_cache(maxsize=None)
def float_case(ocw, null_frac, levels, encoding="nan_zero"):
    """-> (case, f0, f1, a-priori shift): pyramid_any_oracle.float_pyr_case -- non-integral pixels, the nulls NaN in image 0"""
    from mimc3_amd import api
    from pyramid_any_oracle import float_pyr_case
    c, f0, f1 = float_pyr_case(ocw, null_frac, 9900 + ocw + int(100 * null_frac) + levels, levels, encoding)
    return c, f0, f1, api.prior_shift(c.xyuvav, c.dt, c.mpp)


def float_oracle_case():
    """-> (case, f0, f1, shift, ocw, R, levels) of the one case compared with pyramid_search_any"""
    c, f0, f1, shift = float_case(10, 0.03, 3)
    return c, f0, f1, shift, 10, R, 3
