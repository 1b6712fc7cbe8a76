"""Fixtures of the exhaustive search beyond +-15 px on 8-bit pairs on the matrix cores (mimc3_match_ncc_wide_class,
match_wide_u8_kernel.hip) that the CPU and GPU tests share: the kernel's layout in Python terms, the (ocw, R) table -- the smallest
shapes at which a grid of 32 x 32 cell tiles can go wrong -- and 8-bit fixtures with PLACED nulls and statuses: the 12 points of
full_chip_u8_common.u8_case (search boxes that do not overlap: every point's pattern is its own), doctored further so that one launch
holds every kind of point.  The oracle is tests/full_any_oracle.c (full_any_common.full_any, tail_from_surface)."""
import functools

import numpy as np

import full_chip_u8_common as fu
from full_any_common import full_any
from full_multi_common import periodic_pair

PATH, FLOAT_PATH = "u8_mfma_wide", "f32g_wide"
MAX_OCW, R_MIN, R_MAX = 80, 16, 47


def _entry_exists():
    """every test of the three files needs the entry: without it they fail here, at the missing symbol"""
    from mimc3_amd import api
    return api.wide_class_max_radius(MAX_OCW) == R_MAX and hasattr(api.Context, "match_ncc_wide_class")


assert _entry_exists()
SIX = fu.SIX

# R: 16 (S = 33: one cell column and row in the second tile), 23 (S = 47: the second 16-column group), 31 | 32 (S = 63 | 65: two tiles
# one column short, then a third tile of one column), 47 (S = 95: one column short of 3 x 3)
RADII = (16, 23, 31, 32, 47)
# ocw: 1, 7, 16, both sides of the KCW class edges (24 | 25, 56 | 57) and of the single table query's limit (44 | 45), 80
OCWS = (1, 7, 16, 24, 25, 44, 45, 56, 57, 80)
# every R at ocw 7 and 16, every ocw at R 16 and R 47, ocw 80 at R 32
CASES = sorted({(o, r) for o in (7, 16) for r in RADII} | {(o, r) for o in OCWS for r in (16, 47)} | {(80, 32)})
# mode 1 at the six, against match_ncc_wide itself: ocw 7 and 16 at every R, ocw 32 at R 47, ocw 40 at R 39
SIX_CASES = [(o, r) for o in (7, 16) for r in RADII] + [(32, 47), (40, 39)]
OUTSIDE_CASES = [(o, r) for o, r in CASES if o not in SIX]
ORACLE_POINTS_BIG = (0, 1, 2, 4, 6, 7, 8, 10)          # at ocw >= 45 the oracle runs on 8 points: one of every kind

# the points of a fixture by kind (0..5 are u8_case's: box only, chip only, both)
G4, G3CHIP, G3BOX, CLEAN, OUTSIDE, ONE_TILE = 6, 7, 8, 9, 10, 11


# ---- the layout (match_wide_u8_kernel.hip wide_u8_layout) ----
def layout(ocw, R):
    """-> (K chunks per chip row, cell tiles per axis, threads per workgroup, dynamic LDS bytes), or None out of range"""
    if not (1 <= ocw <= MAX_OCW and R_MIN <= R <= R_MAX):
        return None
    cw = 2 * ocw + 1
    kw = cw + 31
    kcw = (cw + 15 + 63) // 64
    rdw, sw = 16 + 64 * kcw, (kw + 15) & ~15
    pw0 = max(rdw, sw)
    pw = pw0 if (pw0 // 16) & 1 else pw0 + 16
    ntr = (kw + 15) // 16
    cp = max((cw + 15 + 3) & ~3, 64 * kcw)
    chb = (16 + (cw + 1) * cp + 16 + 15) & ~15
    off_ch = (max((16 * ntr + 1) * pw, 1280) + 15) & ~15        # (the tile; the 1,280-byte bit plane of the candidate tail takes its bytes)
    S = 2 * R + 1
    return kcw, (S + 31) // 32, 128, off_ch + chb + ((S * 96 * 4 + 15) & ~15)


# ---- fixtures ----
def _fixture(ocw, R, swap, with_shift, saturated):
    c, i0, i1, sh = fu.u8_case(ocw, R, "placed", swap, with_shift, saturated)
    i0, i1 = i0.copy(), i1.copy()
    u, v, cu, cv = fu.geometry(c, sh, swap)
    chip_img, box_img = (i1, i0) if swap else (i0, i1)
    h = ocw + R
    # -4: the chip of point G4 copied to the border of its range, su = +R (the last, partial tile column), sv = 3: NCC = 1 there
    g = G4
    box_img[cv[g] + 3 - ocw:cv[g] + 3 + ocw + 1, cu[g] + R - ocw:cu[g] + R + ocw + 1] = chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
    # -3 by the chip rule, -3 by the box rule (the chip stays as it is)
    g = G3CHIP; chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 0
    g = G3BOX; box_img[cv[g] - h:cv[g] + h + 1, cu[g] - h:cu[g] + h + 1] = 0
    # one null one column outside the box, in a row of the box: inside the last tile's reach, never read by the definition
    g = OUTSIDE; box_img[cv[g] + 1, cu[g] + h + 1] = 0
    # one null in the box that lies inside the window of tile (0, 0) and of no other (box pixel (3, 5): the other tiles start at 32)
    g = ONE_TILE; box_img[cv[g] - h + 5, cu[g] - h + 3] = 0
    sgn = -1 if swap else 1
    off = np.ascontiguousarray(sgn * np.asarray(c.offset), np.int32)
    shift = None if sh is None else np.ascontiguousarray(sgn * np.asarray(sh), np.int32)
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    f = dict(c=c, i0=np.ascontiguousarray(i0, np.float32), i1=np.ascontiguousarray(i1, np.float32), xy=xy, off=off, shift=shift,
             case_shift=sh, ocw=ocw, R=R, swap=swap, what=f"ocw {ocw} R {R} swap {swap} shift {with_shift} saturated {saturated}")
    for a in (f["i0"], f["i1"], xy, off) + (() if shift is None else (shift,)):
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=4)
def fixture(ocw, R, swap=False, with_shift=True, saturated=0):
    """-> dict(c, i0, i1, xy, off, shift, ocw, R, swap, what): the arrays as the call takes them (swapped: offset and shift negated)"""
    return _fixture(ocw, R, swap, with_shift, saturated)


def kinds(f):
    """Per point of a fixture, from its pixels alone -> (clean bool[N], dirty bool[N], refused-by-chip bool[N], refused-by-box bool[N]):
    clean / dirty = no null / a null in chip or box, of the points the validity rule (more than 0.8 nulls) lets through"""
    c, ocw, R = f["c"], f["ocw"], f["R"]
    nc, nb = fu.null_counts(c, f["i0"], f["i1"], f["case_shift"], ocw, R, f["swap"])
    r3c = nc / float((2 * ocw + 1) ** 2) > 0.8
    r3b = nb / float((2 * (ocw + R) + 1) ** 2) > 0.8
    ok = ~(r3c | r3b)
    return ok & (nc == 0) & (nb == 0), ok & ((nc > 0) | (nb > 0)), r3c, r3b


def oracle_points(ocw):
    return np.array(ORACLE_POINTS_BIG if ocw >= 45 else range(fu.DIMX * fu.DIMY))


@functools.lru_cache(maxsize=4)
def oracle(ocw, R, swap=False, with_shift=True, saturated=0):
    """The CPU oracle on oracle_points(ocw) of the fixture -> (points, record, surfaces)"""
    f = fixture(ocw, R, swap, with_shift, saturated)
    pts = oracle_points(ocw)
    rec, _, surf, _ = full_any(f["i0"], f["i1"], f["xy"][pts], f["off"], ocw, R, 0, shift=None if f["shift"] is None else f["shift"][pts], swap=swap)
    return pts, rec, surf


def all_fixtures():
    """(ocw, R, swap, with_shift, saturated) of every placed-null fixture a GPU test uses"""
    out = {(o, r, False, True, 0) for o, r in CASES} | {(o, r, False, True, 0) for o, r in SIX_CASES}
    out |= {(16, 23, True, True, 0), (16, 23, False, False, 0), (10, 24, True, True, 0), (57, 16, True, True, 0), (16, 24, False, True, 0)}
    out |= {(o, r, False, True, 1) for o, r in SATURATED}
    return sorted(out)


SATURATED = ((44, 16), (45, 16), (80, 16), (80, 47))       # 255 everywhere but a few pixels: the integer bounds, the sub-box table sums

# ---- seams: periodic pairs (i0 == i1 of period pu x pv: cells a period apart have identical integer sums, bit-equal NCC = 1) at
#      ocw 7, R 47 (S = 95, tiles at cells 0, 32, 64).  Maxima at the cells x = 47 + i pu, y = 47 + j pv ----
SEAM_OCW, SEAM_R = 7, 47
SEAM_PERIODS = ((16, 16), (15, 17))      # maxima at x, y in {15, 31, 47, 63, 79}; at x in {2, 17, 32, ...}, y in {13, 30, 47, 64, 81}


# the plateau form needs a chip of whole periods (15 px at ocw 7): its flat tops lie at the cells y = R + 15 j and the next one --
# (R, y) = (46, 31): 31 | 32; (33, 63): 63 | 64
PLATEAU_PERIOD = (15, 15)
SEAM_PLATEAUS = ((46, 31), (33, 63))


def seam_pair(pu, pv, plateau):
    """-> (i0, i1, xy): full_multi_common.periodic_pair; plateau: the maxima are flat over sv = 0, 1 (mod pv)"""
    return periodic_pair(pu, pv, plateau)


def maxima_cells(period, R=SEAM_R):
    S = 2 * R + 1
    return [x for x in range(1, S - 1) if (x - R) % period == 0]
