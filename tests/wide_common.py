"""Fixtures of the exhaustive search beyond +-15 px (mimc3_match_ncc_wide) that the CPU and GPU tests share: the case table -- the
smallest shapes at which match_wide_kernel.hip can go wrong -- and the pairs, each doctored so that it holds a status -3 and a status -4
point next to its fitted ones.  The oracle is tests/full_any_oracle.c (full_any_common.full_any, tail_from_surface), which takes R at
run time without a cap."""
import functools

import numpy as np

from full_any_common import encode_nulls, full_any, to_float
from full_dn_common import to_dn16
from full_multi_common import parity_case

# the radius the kernel's LDS layout allows per chip size; the GPU test asserts that the library reports these
MAX_RADIUS = {7: 47, 15: 47, 16: 47, 30: 47, 32: 47, 40: 39}

# (pixel class, null encoding, ocw, R, null fraction, swap, per-point shift)
#   ocw 7 R 16: S = 33, a last group of one cell; R 17 / 18: last groups of three and one; R 47: the cap, 2,280 tasks for 256 threads
#   ocw 16 R 24 with 10 % nulls: clean and dirty workgroups in one launch
#   ocw 32 and ocw 40 at their largest radius: the largest LDS layouts (158,464 and 161,856 bytes)
# R <= 18 (SMALL_R): full_multi_common.parity_case's 214 x 224 pair with its blob nulls, as float_case / dn16_case make it.  There a box
# is 47-51 px wide and about half the points keep chip and box free of excluded pixels.  From R 24 on a box is 81-159 px wide and on
# that pair every one of them holds a blob or hangs over the image edge: every workgroup would take the dirty body.  Those cases get a
# pair of their own (_big_pair): the same texture recipe on an image large enough to hold every box, with the nulls PLACED -- a
# vertical strip that the boxes of the two left grid columns reach and the others do not (null fraction = its share of the search
# image), and a 3 x 3 blob in one chip -- so that one launch holds several clean and several dirty workgroups
# (tests/test_wide_cpu.py states the counts).
SMALL_R = 18
CASES = [
    ("u8", None, 7, 16, 0.03, False, True),
    ("u16", None, 7, 17, 0.03, False, False),
    ("u8", None, 7, 18, 0.03, True, True),
    ("u16", None, 7, 47, 0.03, False, True),
    ("u8", None, 16, 24, 0.10, False, True),
    ("u16", None, 32, MAX_RADIUS[32], 0.03, False, True),
    ("u8", None, 40, MAX_RADIUS[40], 0.03, False, True),
    ("float", "zero", 7, 16, 0.03, False, True),
    ("float", "nan_zero", 7, 17, 0.03, True, True),
    ("float", "m9999_nan", 7, 18, 0.03, False, False),
    ("wide", "zero", 7, 47, 0.03, False, True),
    ("wide", "nan_zero", 16, 24, 0.10, False, True),
    ("wide", "m9999_nan", 32, MAX_RADIUS[32], 0.03, False, True),
    ("float", "zero", 40, MAX_RADIUS[40], 0.03, False, True),
    ("float", "m9999_nan", 16, 24, 0.10, True, True),
]
EXACT = ("u8", "u16")


def case_id(case):
    kind, enc, ocw, R, nf, swap, sh = case
    return f"{kind}{'-' + enc if enc else ''}-ocw{ocw}-R{R}" + ("-swap" if swap else "") + ("" if sh else "-noshift")


def _plant(chip_img, win_img, xy, off, shift, ocw, R, g3, g3box=None):
    """Doctor a pair in place so that it holds the statuses a test wants to see.
    -4: the chip of one point is copied into the search image at offset (+R, dv) from its search centre -- NCC = 1 on the border (the chip's nulls go with it:
        they are excluded on both sides);
    -3: the chip of another point is set to 0 (every pixel below MIN_DN, whatever the null encoding): the chip rule;
    -3: (g3box given) the whole search box of a third point is set to 0 while its chip stays as it is: the box rule, over the staging
        whose rows are wider than the box.  -> (g4, g3)"""
    H, W = chip_img.shape
    n = xy.shape[0]
    g4 = None
    for g in range(n):
        u0, v0 = int(xy[g, 2]), int(xy[g, 3])
        bu = u0 + int(off[0]) + (int(shift[g, 0]) if shift is not None else 0)
        bv = v0 + int(off[1]) + (int(shift[g, 1]) if shift is not None else 0)
        cu, cv, h = bu + R, bv + 3, R + ocw
        chip = chip_img[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1]
        # (the whole box inside the image: a window that hangs far over the edge keeps a handful of pixels, and such a cell can reach 1)
        if bu - h >= 0 and bu + h < W and bv - h >= 0 and bv + h < H and (np.nan_to_num(chip, nan=0.0) > 0).mean() > 0.5:
            win_img[cv - ocw:cv + ocw + 1, cu - ocw:cu + ocw + 1] = chip
            g4 = g
            break
    assert g4 is not None and g4 not in (g3, g3box)
    u0, v0 = int(xy[g3, 2]), int(xy[g3, 3])
    chip_img[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1] = 0.0
    if g3box is not None:
        bu = int(xy[g3box, 2]) + int(off[0]) + (int(shift[g3box, 0]) if shift is not None else 0)
        bv = int(xy[g3box, 3]) + int(off[1]) + (int(shift[g3box, 1]) if shift is not None else 0)
        h = R + ocw
        win_img[max(bv - h, 0):bv + h + 1, max(bu - h, 0):bu + h + 1] = 0.0
    return g4


BIG_STEP = 32                            # grid spacing (px) of _big_pair


def _big_pair(ocw, R, nf, swap):
    """The 8-bit pair of a case with R > SMALL_R: parity_case's recipe (a nearly white texture, +-2 DN of noise, displaced by (3, -2),
    offset (1, -1), a 5 x 4 grid) on an image that holds every search box, without blobs; then 0 = null in a vertical strip of the
    search image, nf of its width, which only the boxes of grid columns 0 and 1 reach, and in a 3 x 3 block at the centre of point 11's
    chip (two rows below point 0, whose chip is the one copied for the status -4).  -> (case, i0, i1, a-priori shift)"""
    from mimc3_amd import api, synth
    m = R + ocw + 8
    c = synth.make_small(seed=7300 + ocw + R, shift=(3, -2), angle_deg=40.0, ocw=ocw, speed=700.0, h=2 * m + 3 * BIG_STEP,
                         w=2 * m + 4 * BIG_STEP, dimx=5, dimy=4, noise_dn=2, null_frac=0.0, offset=(1, -1), sigma=0.3, margin=m)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    i0, i1 = c.i0.copy(), c.i1.copy()
    chip_img, win_img = (i1, i0) if swap else (i0, i1)
    sgn = -1 if swap else 1
    left = c.xyuvav[:, 2].astype(np.int64) + sgn * (int(c.offset[0]) + shift[:, 0]) - (R + ocw)       # the boxes' left edges
    col = np.arange(c.n) % 5
    x0, x1 = int(left[col == 1].max()) + 2, int(left[col == 2].min()) - 2
    x1 = min(x1, x0 + max(int(round(nf * win_img.shape[1])), 4))
    assert x1 - x0 >= 4
    win_img[:, x0:x1] = 0
    u, v = int(c.xyuvav[11, 2]), int(c.xyuvav[11, 3])
    chip_img[v - 1:v + 2, u - 1:u + 2] = 0
    return c, i0, i1, shift


def _amplitude(shape):
    """full_any_common.wide_case's smooth amplitude field, six decades over 160 px"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return np.power(10.0, 3.0 * np.sin(2 * np.pi * (xx + 0.6 * yy) / 160.0)).astype(np.float32)


def _pair(kind, enc, ocw, R, nf, swap):
    """-> (case, i0, i1, a-priori shift) in the case's pixel class and null encoding"""
    if R <= SMALL_R:
        c, shift = parity_case(ocw, nf, R, dimx=5, dimy=4)
        b0, b1 = c.i0, c.i1
    else:
        c, b0, b1, shift = _big_pair(ocw, R, nf, swap)
    if kind == "u8":
        return c, b0.copy(), b1.copy(), shift
    if kind == "u16":
        return c, to_dn16(b0, 1000 + ocw), to_dn16(b1, 2000 + ocw), shift
    f0, f1 = to_float(b0, 3000 + ocw), to_float(b1, 4000 + ocw)
    if kind == "wide":
        amp = _amplitude(f0.shape)
        f0, f1 = (f0 * amp).astype(np.float32), (f1 * amp).astype(np.float32)
    f0, f1 = encode_nulls(f0, f1, enc)
    return c, np.ascontiguousarray(f0), np.ascontiguousarray(f1), shift


@functools.lru_cache(maxsize=None)
def _fixture(case):
    kind, enc, ocw, R, nf, swap, use_shift = case
    c, i0, i1, shift = _pair(kind, enc, ocw, R, nf, swap)
    sgn = -1 if swap else 1
    off = sgn * np.asarray(c.offset, np.int32)
    shift = np.ascontiguousarray(sgn * shift, np.int32) if use_shift else None
    if use_shift:
        assert (shift != 0).any()
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    i0, i1 = np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32)
    # small pair: the chip rule at the last point, the box rule at point 12; big pair: the chip rule at point 15 (grid column 0)
    g3, g3box = (c.n - 1, 12) if R <= SMALL_R else (15, None)
    g4 = _plant(i1 if swap else i0, i0 if swap else i1, xy, off, shift, ocw, R, g3, g3box)
    for a in (i0, i1, xy, off) + (() if shift is None else (shift,)):
        a.setflags(write=False)
    return dict(i0=i0, i1=i1, xy=xy, off=off, shift=shift, ocw=ocw, R=R, swap=swap, g4=g4, g3=g3, g3box=g3box, exact=kind in EXACT, what=case_id(case))


def fixture(case):
    """-> dict(i0, i1, xy, off, shift, ocw, R, swap, g4, g3, exact, what); the arrays are shared and read-only"""
    return _fixture(tuple(case))


@functools.lru_cache(maxsize=None)
def _oracle(case):
    f = _fixture(case)
    rec, _, surf, nlm = full_any(f["i0"], f["i1"], f["xy"], f["off"], f["ocw"], f["R"], 0, shift=f["shift"], swap=f["swap"])
    for a in (rec, surf, nlm):
        a.setflags(write=False)
    return rec, surf, nlm


def oracle(case):
    """The CPU oracle of a case, computed once per process -> (record, surfaces, local-maximum counts)"""
    return _oracle(tuple(case))


def body_counts(f, rec):
    """Of the points the validity rule lets through (status != -3): how many have no excluded pixel (not >= 1e-10: 0, negatives, NaN;
    outside the image) in chip and box -- the kernel's clean body -- and how many have one -- the dirty body -> (clean, dirty)"""
    chip_img, win_img = (f["i1"], f["i0"]) if f["swap"] else (f["i0"], f["i1"])
    ocw, h = f["ocw"], f["R"] + f["ocw"]
    H, W = win_img.shape
    ex = np.ones((H + 2 * h + 64, W + 2 * h + 64), bool)
    p = h + 32
    ex[p:p + H, p:p + W] = ~(win_img.astype(np.float64) >= 1e-10)
    exc = ~(chip_img.astype(np.float64) >= 1e-10)
    clean = dirty = 0
    for g in range(f["xy"].shape[0]):
        if rec[g, 2] == -3:
            continue
        u0, v0 = int(f["xy"][g, 2]), int(f["xy"][g, 3])
        bu = u0 + int(f["off"][0]) + (int(f["shift"][g, 0]) if f["shift"] is not None else 0) + p
        bv = v0 + int(f["off"][1]) + (int(f["shift"][g, 1]) if f["shift"] is not None else 0) + p
        bad = exc[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1].any() or ex[bv - h:bv + h + 1, bu - h:bu + h + 1].any()
        clean, dirty = clean + (not bad), dirty + bool(bad)
    return clean, dirty


def status_counts(rec):
    """-> (points with a fit, status -4 points, status -3 points, status -2 points)"""
    st = rec[:, 2]
    return int(np.isfinite(rec[:, 0]).sum()), int((st == -4).sum()), int((st == -3).sum()), int((st == -2).sum())


# ---- the crafted pair: a periodic 8-bit texture whose surface at ocw 7, R 18 has nine interior local maxima a period (9 x 11 px) apart,
#      all exactly tied at NCC = 1, and the same value on the border cells su = -18: the first-wins arg-max is a border cell (-4) ----
CRAFT_OCW, CRAFT_R, CRAFT_PERIOD = 7, 18, (9, 11)


# ---- what it is for: a pair displaced by (34, -27) px from the zero shift ----
FAR_TRUE, FAR_OCW, FAR_R = (34, -27), 16, 40


def far_case():
    """A 300 x 320 8-bit pair displaced by FAR_TRUE, +-2 DN of noise, a 4 x 3 grid -> case"""
    from mimc3_amd import synth
    return synth.make_small(seed=4711, shift=FAR_TRUE, ocw=FAR_OCW, h=300, w=320, dimx=4, dimy=3, noise_dn=2, margin=70)


# ---- a plain numpy restatement of the tail's decisions (not its fits) on a surface val[x][y] ----
def tail_decisions_py(val, npeaks):
    """-> (status or None for a fit, arg-max k or -1, the k of the first npeaks ranked local maxima)"""
    from full_multi_common import ranked_local_maxima_py
    S = val.shape[0]
    R = S // 2
    flat = val.ravel()                                       # k = x S + y
    fin = np.isfinite(flat)
    ranked = ranked_local_maxima_py(val)[:npeaks]
    if not fin.any():
        return -2, -1, ranked
    best = np.where(fin, flat, -np.inf)
    k = int(np.argmax(best))                                 # numpy's arg-max is first-wins
    su, sv = k // S - R, k % S - R
    return (-4 if max(abs(su), abs(sv)) == R else None), k, ranked
