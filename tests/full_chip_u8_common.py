"""Test infrastructure of the exhaustive search on 8-bit pairs at any chip size on the matrix cores (mimc3_match_ncc_full_chip_class,
match_full_chip_u8_kernel.hip): the kernel's layout in Python terms, the chip sizes on both sides of every change of it, and 8-bit
fixtures with PLACED nulls -- 12 points whose search boxes do not overlap, so that every point's null pattern is its own: two points
with a null in the box only (its last row, its last column), two with a null in the chip only (its first row, its last row), two with
nulls on both sides, six clean.  tests/test_full_chip_u8_cpu.py counts every fixture of the GPU tests without a device."""
import functools

import numpy as np

from value_limit_common import top_of_class

PATH = "u8_mfma_chip"
MAX_OCW = 80
SIX = (7, 15, 16, 30, 32, 40)
DIMX, DIMY = 4, 3
BOX_ONLY, CHIP_ONLY, BOTH = (0, 1), (2, 3), (4, 5)      # the points of a placed-null fixture, by what holds their nulls


# ---- the layout (match_full_chip_u8_kernel.hip chip_u8_layout) ----
def layout(ocw):
    """-> dict: KCW K chunks of 64 window columns per chip row, NTR 16-row tiles and KCV K chunks of the box sums, lds dynamic LDS bytes"""
    cw = 2 * ocw + 1
    kw = cw + 31
    kcw = (cw + 15 + 63) // 64
    rdw, sw = 16 + 64 * kcw, (kw + 15) & ~15
    pw0 = max(rdw, sw)
    pw = pw0 if (pw0 // 16) & 1 else pw0 + 16
    ntr = (kw + 15) // 16
    cp = max((cw + 15 + 3) & ~3, 64 * kcw)
    chb = (16 + (cw + 1) * cp + 16 + 15) & ~15
    off_ch = (max((16 * ntr + 1) * pw, 4 * 32 * 33) + 15) & ~15
    return dict(CW=cw, KCW=kcw, NTR=ntr, KCV=(ntr + 3) // 4, lds=off_ch + chb)


def layout_tuple(ocw):
    L = layout(ocw)
    return (L["KCW"], L["NTR"], L["KCV"], L["lds"]) if 1 <= ocw <= MAX_OCW else None


def boundaries(query=layout_tuple):
    """The chip sizes on both sides of every change of KCW, NTR or KCV over ocw 1..80, from `query` (the library's on the GPU side)
    -> {field: [(ocw below, ocw above), ...]}"""
    out = {"KCW": [], "NTR": [], "KCV": []}
    for ocw in range(1, MAX_OCW):
        a, b = query(ocw), query(ocw + 1)
        for i, f in enumerate(("KCW", "NTR", "KCV")):
            if a[i] != b[i]:
                out[f].append((ocw, ocw + 1))
    return out


# ---- fixtures ----
@functools.lru_cache(maxsize=None)
def _base(ocw, radius):
    """A null-free 8-bit pair on a nearly white texture (full_multi_common.parity_case's) and a 4 x 3 grid whose search boxes lie
    2 (ocw + radius) + 15 px apart: no pixel belongs to two points' boxes or chips"""
    from mimc3_amd import api, synth
    h = ocw + radius
    step, margin = 2 * h + 15, h + 12
    c = synth.make_small(seed=7300 + ocw, shift=(3, -2), angle_deg=40.0, ocw=ocw, speed=700.0, h=2 * margin + (DIMY - 1) * step + 1,
                         w=2 * margin + (DIMX - 1) * step + 1, dimx=DIMX, dimy=DIMY, noise_dn=2, null_frac=0.0, offset=(1, -1), sigma=0.3,
                         margin=margin)
    i0, i1 = np.where(c.i0 == 0, 1, c.i0).astype(np.float32), np.where(c.i1 == 0, 1, c.i1).astype(np.float32)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    for a in (i0, i1, shift, c.xyuvav):
        a.setflags(write=False)
    return c, i0, i1, shift


def geometry(c, shift, swap):
    """-> (u, v, cu, cv) int arrays: chip centres and search centres of the call that run() makes (swapped: offset and shift negated)"""
    sgn = -1 if swap else 1
    u, v = c.xyuvav[:, 2].astype(np.int64), c.xyuvav[:, 3].astype(np.int64)
    sh = np.zeros((c.n, 2), np.int64) if shift is None else np.asarray(shift, np.int64)
    return u, v, u + sgn * (int(c.offset[0]) + sh[:, 0]), v + sgn * (int(c.offset[1]) + sh[:, 1])


def u8_case(ocw, radius, nulls="placed", swap=False, with_shift=True, saturated=0):
    """-> (case, i0, i1, shift or None).  nulls: "placed" (see the module's text; for the direction of `swap`), "none", "all" (every
    point: a null in its box, every other one also in its chip).  saturated: a spread s > 0 presses the pair against 255
    (value_limit_common.top_of_class: pixels 255 - s .. 255), the nulls placed afterwards."""
    c, b0, b1, shift = _base(ocw, radius)
    i0, i1 = b0.copy(), b1.copy()
    if saturated:
        i0, i1 = top_of_class(i0, 255, saturated).copy(), top_of_class(i1, 255, saturated).copy()
    sh = shift if with_shift else None
    u, v, cu, cv = geometry(c, sh, swap)
    chip_img, box_img = (i1, i0) if swap else (i0, i1)
    h = ocw + radius
    if nulls == "placed":
        g = BOX_ONLY[0]; box_img[cv[g] + h, cu[g] - 3] = 0              # the last box row
        g = BOX_ONLY[1]; box_img[cv[g] + 2, cu[g] + h] = 0              # the last box column
        g = CHIP_ONLY[0]; chip_img[v[g] - ocw, u[g]] = 0                # the first chip row
        g = CHIP_ONLY[1]; chip_img[v[g] + ocw, u[g] + ocw] = 0          # the last chip row (and column)
        g = BOTH[0]; chip_img[v[g], u[g] - 1] = 0; box_img[cv[g] + 1, cu[g]] = 0
        g = BOTH[1]; chip_img[v[g] - 1, u[g] - ocw] = 0; box_img[cv[g] - h, cu[g] + 1] = 0
    elif nulls == "all":
        for g in range(c.n):
            box_img[cv[g] - h + (7 * g) % (2 * h + 1), cu[g] + h - (5 * g) % (2 * h + 1)] = 0
            if g & 1:
                chip_img[v[g] + ocw - (3 * g) % (2 * ocw + 1), u[g] - ocw + (11 * g) % (2 * ocw + 1)] = 0
    else:
        assert nulls == "none"
    return c, np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32), sh


def null_counts(c, i0, i1, shift, ocw, radius, swap):
    """per point the nulls of its chip and of its search box (pixels outside the image are the planes' zero border: nulls) -> two int arrays"""
    u, v, cu, cv = geometry(c, shift, swap)
    chip_img, box_img = (i1, i0) if swap else (i0, i1)
    H, W = box_img.shape
    h = ocw + radius
    nc, nb = [], []
    for g in range(c.n):
        nc.append(int((chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] == 0).sum()))
        y0, y1, x0, x1 = max(cv[g] - h, 0), min(cv[g] + h + 1, H), max(cu[g] - h, 0), min(cu[g] + h + 1, W)
        inside = max(y1 - y0, 0) * max(x1 - x0, 0)
        nb.append((2 * h + 1) ** 2 - inside + int((box_img[y0:y1, x0:x1] == 0).sum()))
    return np.array(nc), np.array(nb)


# ---- every placed-null fixture a GPU test uses: (ocw, R, swap, with_shift, saturated spread) ----
RADII = ((10, 1), (10, 4), (10, 7), (10, 15), (80, 15), (80, 1))
SATURATED_OCW = (44, 45, 80)


def size_cases(query=layout_tuple):
    """(ocw, R) of the chip-size cases: 1, 2, 3 (a chip row below one dword pair, both values of CW mod 4), 10, 11, 14, both sides of
    every change of the layout, 60 and 80; R 15 except at the small chips, which alternate"""
    ocws = {1, 2, 3, 10, 11, 14, 60, 80}
    for pairs in boundaries(query).values():
        for a, b in pairs:
            ocws |= {a, b}
    return [(o, 15 if o > 3 or o == 2 else 4) for o in sorted(ocws)]


def all_fixtures():
    out = {(o, r, False, True, 0) for o, r in size_cases()} | {(o, r, False, True, 0) for o, r in RADII}
    out |= {(10, 7, True, True, 0), (57, 15, True, True, 0), (10, 7, False, False, 0), (10, 7, True, False, 0)}
    out |= {(o, 15, False, True, 1) for o in SATURATED_OCW} | {(o, 15, False, True, 3) for o in SATURATED_OCW}
    out |= {(o, 15 if o != 16 else 7, False, True, 0) for o in (7, 16, 40)}
    return sorted(out)
