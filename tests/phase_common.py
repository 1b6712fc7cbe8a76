"""Fixtures that reach every pixel phase of chip and window origin, shared by tests/test_pixel_phases_cpu.py and tests/test_pixel_phases.py.

Every tiled kernel stages chip and window rows as aligned dwords and shifts them by the phase of the row's first column: `& 3` for
the 8-bit planes, `& 1` for the 16-bit ones (match_mx_kernel.hip, match_px_kernel.hip, match_full_u16_kernel.hip), 16-byte slots in the
f32 search kernels.  The grids of synth.make_grid reach one or two of those phases; the grids here have odd spacings, so one launch
holds all four chip phases, and every call is repeated at four control-point offsets, which moves the window through its four.

Here: the phase arithmetic restated in numpy (`phases`), one pair and one grid per chip size with nulls planted per point
(`fixture`), the cells a fixture reaches (`coverage`), and the same grid at fractional coordinates (`fractional`: the reference
truncates u and v toward zero, MIMC_module.c:822-823)."""
import collections
import functools
import types

import numpy as np

from mimc3_amd import synth
from u8_advance_common import BORDER, box, classify, null_table

OCWS = (7, 15, 16, 30, 32, 40)
DIMX = DIMY = 8
# the a-priori per grid row: |lu| 10, 11, 12, 13 in either direction along u -- both parities of |lu|, so both values of Dx2 mod 4.
# (get_uv_pivot's corridor is speed dt aw_sf / mpp / 365 + aw_cre + 1 long and advances one pixel in u per pivot at these angles)
ROW_SPEED = (90.0, 280.0, 490.0, 700.0, 90.0, 280.0, 490.0, 700.0)
ROW_ANGLE = (25.0, 25.0, 25.0, 25.0, 155.0, 155.0, 155.0, 155.0)
LU_MAX, LV_MAX = 13, 6
TRUE_SHIFT = (3, -2)
OFFSETS = ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1))        # the four window phases, and once a row down
SEARCH_R = 7
NULL_CLASSES = ("none", "chip", "window", "both")
KINDS = ("u8", "9bit", "12bit", "eighths", "16bit")
BRIGHT = 500.0                                            # 9-bit pairs: a pixel that takes its chip or window out of a local 8-bit range
FRACTIONS = (0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -20)
BRIGHT_POINTS = tuple(range(5, DIMX * DIMY, 16))              # the points of a 9-bit pair that get the bright pixel


def trunc(xy):
    """(u0, v0) as every kernel's point header takes them: C's conversion to int, toward zero"""
    return np.trunc(xy[:, 2]).astype(np.int64), np.trunc(xy[:, 3]).astype(np.int64)


def phases(xy, offset, off, uv, ocw, shift=None, radius=None):
    """Per point the phases of the first column and row the kernels stage.  The planes' border of 256 pixels is a multiple of 4, so these
    are the kernels' own `& 3` values (the u16 kernels see `& 1` of the same numbers).
      cph, cpv: the chip's first column and row, (u0 - ocw) & 3
      wph, wpv: the window's -- the DLC matcher's (radius None: off, uv are the pivots' CSR arrays), u0 + off_u - (|lu| + ocw + 2), or the
                search box's, u0 + off_u + shift_u - R - ocw
      eph, epv (DLC only): the row end, (wph + Dx2) & 3 with Dx2 = 2 (|lu| + ocw + 2) + 1; dx4, dy4: Dx2 & 3"""
    u0, v0 = trunc(xy)
    res = dict(cph=(u0 - ocw) & 3, cpv=(v0 - ocw) & 3)
    if radius is None:
        last = np.asarray(uv, np.int64)[np.asarray(off, np.int64)[1:] - 1]
        dx2, dy2 = np.abs(last[:, 0]) + ocw + 2, np.abs(last[:, 1]) + ocw + 2
        wu, wv = u0 + int(offset[0]) - dx2, v0 + int(offset[1]) - dy2
        res.update(wph=wu & 3, wpv=wv & 3, eph=(wu + 2 * dx2 + 1) & 3, epv=(wv + 2 * dy2 + 1) & 3, dx4=(2 * dx2 + 1) & 3, dy4=(2 * dy2 + 1) & 3)
    else:
        sh = np.zeros((xy.shape[0], 2), np.int64) if shift is None else np.asarray(shift, np.int64)
        res.update(wph=(u0 + int(offset[0]) + sh[:, 0] - radius - ocw) & 3, wpv=(v0 + int(offset[1]) + sh[:, 1] - radius - ocw) & 3)
    return res


def geometry(ocw, reach=None):
    """-> (H, W, first u, first v, spacing in u, in v): odd spacings larger than the largest DLC window plus 4, so that no two windows
    overlap; every window inside the image.  reach (a search radius beyond 16, where the search boxes of that spacing overlap): odd
    spacings larger than the search box of that radius at every offset of OFFSETS and under every a-priori shift, so that no two boxes
    overlap; every box inside the image (a smaller reach leaves the grid as it is)"""
    dx2, dy2 = LU_MAX + ocw + 2, LV_MAX + ocw + 2
    su, sv = 2 * dx2 + 7, 2 * dy2 + 7
    mu, mv = dx2 + 6, dy2 + 6
    if reach is not None:
        hu, hv = reach + ocw + LU_MAX + 3, reach + ocw + LV_MAX + 3              # what a box reaches from its point, either way
        su, sv, mu, mv = max(su, 2 * hu + 3), max(sv, 2 * hv + 3), max(mu, hu + 2), max(mv, hv + 2)
    return 2 * mv + (DIMY - 1) * sv, 2 * mu + (DIMX - 1) * su, mu, mv, su, sv


def grid(ocw, reach=None):
    _, _, mu, mv, su, sv = geometry(ocw, reach)
    iy, ix = np.divmod(np.arange(DIMX * DIMY), DIMX)
    u, v = (mu + su * ix).astype(np.float64), (mv + sv * iy).astype(np.float64)
    speed, ang = np.asarray(ROW_SPEED)[iy], np.deg2rad(np.asarray(ROW_ANGLE))[iy]
    xy = np.stack([u * synth.MPP, -v * synth.MPP, u, v, speed * np.cos(ang), speed * np.sin(ang)], axis=-1)
    return np.ascontiguousarray(xy, np.float64)


def planned_classes(ocw, reach=None):
    """the null class of every point: within each (chip phase, parity of the row's |lu|) group the points cycle through the four"""
    xy = grid(ocw, reach)
    iy, ix = np.divmod(np.arange(DIMX * DIMY), DIMX)
    key = ((trunc(xy)[0] - ocw) & 3) * 2 + (iy & 1)
    cls = np.zeros(xy.shape[0], np.int64)
    for k in range(8):
        g = np.flatnonzero(key == k)
        cls[g] = (np.arange(g.size) + k // 2) % 4
    return cls


def _base(ocw, bits, reach=None):
    H, W = geometry(ocw, reach)[:2]
    return synth.make_pair(H, W, TRUE_SHIFT, 9100 + ocw, noise_dn=2, bits=bits, sigma=1.0)


@functools.lru_cache(maxsize=None)
def fixture(ocw, kind="u8", plan="dlc", reach=None):
    """One pair and one grid per chip size -> namespace (i0, i1, xy, off, uv: the pivots' CSR arrays, ocw, dt, mpp, cls: the planned null
    class per point, kind, plan); read-only arrays, shared among the tests.

    Nulls are single pixels, planted per point (cls: 0 none, 1 one in the chip, 2 one in the window, 3 both):
      * the chip's null moves through the chip's columns and rows with the point's index (first and last column included);
      * plan "dlc": the window's null sits in the window's middle row, 4 columns inside the window's edge on the side the corridor leads
        away from.  That is outside the chip footprint of every cell the climb can reach (u8_advance_common.axis_geometry: the climb area
        begins |lu| >= 10 columns in), and stays so at every offset of OFFSETS;
      * plan "search": it sits ocw + 4 columns right of the point, a row down: inside the search box of radius SEARCH_R at every offset, with
        and without the a-priori shift.
    kind: "u8" synth.texture; "9bit" the remap of tests/test_match_parity.py's nine_bit_case (150 + 0.8 p), with a pixel of 500 next to
    every 16th point, in chip and window; "12bit"; "eighths" (the 12-bit pair / 8); "16bit".
    reach: the grid of geometry(ocw, reach), for searches of a radius beyond 16 (plan "search" only); a reach below SEARCH_R puts the
    window's null 4 columns right of the point, a row down: at ocw >= 18 inside the search box of every radius from 1 on at every offset,
    with and without the a-priori shift."""
    from oracle.oracle import Oracle
    assert kind in KINDS and plan in ("dlc", "search") and (reach is None or plan == "search")
    i0, i1 = _base(ocw, {"u8": 8, "9bit": 8, "12bit": 12, "eighths": 12, "16bit": 16}[kind], reach)
    if kind == "9bit":
        i0, i1 = (np.round(150.0 + i * 0.8).astype(np.float32) for i in (i0, i1))
    elif kind == "eighths":
        i0, i1 = (i0 / 8).astype(np.float32), (i1 / 8).astype(np.float32)
    H, W = i0.shape
    xy = grid(ocw, reach)
    off, uv = Oracle("port").get_uv_pivot(xy, synth.DT_DAYS, synth.MPP, ocw, H, W)
    last = uv[off[1:] - 1].astype(np.int64)
    u0, v0 = trunc(xy)
    cls = planned_classes(ocw, reach)
    cw = 2 * ocw + 1
    for g in range(xy.shape[0]):
        if kind == "9bit" and g in BRIGHT_POINTS:
            i0[v0[g] + 1, u0[g] - 1] = BRIGHT
            i1[v0[g] - 1, u0[g] + 1] = BRIGHT
        if cls[g] in (1, 3):
            col = (0, cw - 1, (7 * g + 2) % cw, (3 * g + 1) % cw)[(g + g // DIMX) % 4]
            i0[v0[g] - ocw + (5 * g + 3) % cw, u0[g] - ocw + col] = 0.0
        if cls[g] in (2, 3):
            if plan == "dlc":
                dx2 = abs(last[g, 0]) + ocw + 2
                i1[v0[g], u0[g] - dx2 + 4 if last[g, 0] > 0 else u0[g] + dx2 - 1] = 0.0
            else:
                i1[v0[g] + 1, u0[g] + (4 if reach is not None and reach < SEARCH_R else ocw + 4)] = 0.0
    for a in (i0, i1, xy, off, uv, cls):
        a.setflags(write=False)
    return types.SimpleNamespace(i0=i0, i1=i1, xy=xy, off=off, uv=uv, ocw=ocw, dt=synth.DT_DAYS, mpp=synth.MPP, cls=cls, kind=kind, plan=plan,
                                 offset=np.zeros(2, np.int32))


def many_pivot_fixture(ocw, angle=10.0):
    """tests/test_match_parity.py's corridor of about 100 pivots (the forms that stage without tables) on a grid of odd spacings: 4 x 4
    points, one chip phase per column"""
    reach = 100 + ocw + 2
    h, w = (2 * (40 + ocw) + 141 + 3 * 31, 2 * reach + 141 + 3 * 33)
    i0, i1 = synth.make_pair(h, w, (5, -5), 9300 + ocw, noise_dn=2, null_frac=0.02)
    xy = synth.make_grid(4, 4, reach + 20, 40 + ocw + 20, 33, 31, 17000.0, angle_deg=angle)
    return types.SimpleNamespace(i0=i0, i1=i1, xy=xy, ocw=ocw, dt=synth.DT_DAYS, mpp=synth.MPP)


def fractional(xy, seed):
    """the same grid with u, v replaced by trunc + f: f cycles through FRACTIONS, chosen independently for u and v (the seed picks where
    each cycle starts and how the two run against each other)"""
    out = np.array(xy, np.float64)
    n = out.shape[0]
    f = np.asarray(FRACTIONS)
    k = np.arange(n)
    out[:, 2] = np.trunc(out[:, 2]) + f[(k + seed) % 5]
    out[:, 3] = np.trunc(out[:, 3]) + f[(2 * k + k // 5 + 3 * seed) % 5]
    assert np.array_equal(np.trunc(out[:, 2:4]), np.trunc(np.asarray(xy)[:, 2:4]))
    return np.ascontiguousarray(out)


def search_shifts(f):
    """the a-priori shift of every point (api.prior_shift), and None: the two forms every search runs with"""
    from mimc3_amd import api
    return api.prior_shift(f.xy, f.dt, f.mpp), None


def plane_end_points(f, radius):
    """Two points (copies of the fixture's first two, so inside the image) with shifts that put their search box at the end of the
    zero-bordered plane -> (xy [2][6], shift int32[2][2]): the first box ends in the plane's last row, and in its columns 4 .. 1 from
    the last at offset_u 0 .. 3; the second ends 20 rows above the last, and in the last column at offset_u 3.  (The host entries
    require box end < size + BORDER: these are the last boxes they take.)"""
    H, W = f.i0.shape
    xy = np.array(f.xy[:2], np.float64)
    u0, v0 = trunc(xy)
    h = radius + f.ocw
    shift = np.array([[W + BORDER - 1 - 4 - h - u0[0], H + BORDER - 1 - h - v0[0]],
                      [W + BORDER - 1 - 3 - h - u0[1], H + BORDER - 1 - 20 - h - v0[1]]], np.int32)
    return xy, shift


def search_null_class(f, offset, shift, radius, swap=False):
    """per point 0 none, 1 chip only, 2 box only, 3 both -- counted in the images, not read from the plan"""
    chip, win = (f.i1, f.i0) if swap else (f.i0, f.i1)
    Sc, Sw = null_table(chip), null_table(win)
    u0, v0 = trunc(f.xy)
    sh = np.zeros((f.xy.shape[0], 2), np.int64) if shift is None else np.asarray(shift, np.int64)
    ocw, side = f.ocw, 2 * (radius + f.ocw) + 1
    chip_n = box(Sc, u0 - ocw, v0 - ocw, 2 * ocw + 1, 2 * ocw + 1)
    box_n = box(Sw, u0 + int(offset[0]) + sh[:, 0] - radius - ocw, v0 + int(offset[1]) + sh[:, 1] - radius - ocw, side, side)
    return (chip_n > 0) + 2 * (box_n > 0)


def coverage(f, family, radius=SEARCH_R, offsets=OFFSETS):
    """The multiset of cells the fixture's calls reach over `offsets` -> Counter.
      "dlc":    (cph, wph, Dx2 & 3, null class)            "dlc16": the same on the u16 planes' parities, (cph & 1, wph & 1, ...)
      "auto":   (cph, wph, list) with list clean, advance or rest: where u8_classify puts the point (u8_advance_common.classify)
      "search": (cph, wph, null class) with and without the a-priori shift
    Null classes are counted in the images per call (a null planted for one offset may leave the window at another)."""
    cells = collections.Counter()
    for offset in offsets:
        if family == "search":
            for shift in search_shifts(f):
                p = phases(f.xy, offset, None, None, f.ocw, shift=shift, radius=radius)
                cells.update(zip(p["cph"].tolist(), p["wph"].tolist(), search_null_class(f, offset, shift, radius).tolist()))
            continue
        p = phases(f.xy, offset, f.off, f.uv, f.ocw)
        k = classify(f.i0, f.i1, f.xy, offset, f.off, f.uv, f.ocw)
        assert k["takes"].all()
        null = ((k["chip_n"] > 0) + 2 * (k["win_n"] > 0)).tolist()
        if family == "dlc":
            cells.update(zip(p["cph"].tolist(), p["wph"].tolist(), p["dx4"].tolist(), null))
        elif family == "dlc16":
            cells.update(zip((p["cph"] & 1).tolist(), (p["wph"] & 1).tolist(), p["dx4"].tolist(), null))
        elif family == "auto":
            lst = np.where(k["clean"], "clean", np.where(k["advance"], "advance", "rest"))
            cells.update(zip(p["cph"].tolist(), p["wph"].tolist(), lst.tolist()))
        else:
            raise ValueError(family)
    return cells


def coverage_table(f, family, radius=SEARCH_R, offsets=OFFSETS[:4]):
    """the cells as text, one line per (cph, wph), counted over the four offsets in u as tests/test_pixel_phases_cpu.py asserts them:
    what profiles/pixel_phases/ records"""
    cells = coverage(f, family, radius=radius, offsets=offsets)
    keys = sorted({c[2:] for c in cells})
    lines = [f"ocw {f.ocw} {f.kind} {family}" + (f" R {radius}" if family == "search" else "") + ": columns " + " ".join(str(k) for k in keys)]
    for a, b in sorted({c[:2] for c in cells}):
        lines.append(f"  cph {a} wph {b}: " + " ".join(f"{cells[(a, b) + k]:3d}" for k in keys))
    return "\n".join(lines)


assert BORDER % 4 == 0
