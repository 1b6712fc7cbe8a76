"""Fixtures of the exhaustive search beyond +-15 px on scaled-integer pairs (12-bit DN, filtered 8-bit pairs) on the matrix cores
(mimc3_match_ncc_wide_planes, match_wide_u16_kernel.hip) that the CPU and GPU tests share: the kernel's layout and radius limit in Python
terms, the (ocw, R) table drawn from them, and 12-bit fixtures with PLACED nulls and statuses -- the 12 points of
tests/wide_u8_common.py (search boxes that do not overlap), their pixels mapped to 12 bits with full_chip_u16_common.spread12 FIRST and
every null, the -3 areas and the -4 chip copy planted on the 12-bit images afterwards: a copy made before a position-dependent spread is
no longer a copy.  The oracle is tests/full_any_oracle.c (full_any_common.full_any, tail_from_surface)."""
import functools

import numpy as np

import full_chip_u8_common as fu
import wide_u8_common as wu
from full_any_common import full_any
from full_chip_u16_common import spread12
from value_limit_common import top_of_class

PATH, U8_PATH, FLOAT_PATH, CHIP_PATH = "u16_mfma_wide", "u8_mfma_wide", "f32g_wide", "u16_mfma_chip"
MAX_OCW, R_MIN, R_MAX, LDS_MAX = 80, 16, 47, 160 * 1024


def _entry_exists():
    """every test of the three files needs the entry: without it they fail here, at the missing symbol"""
    from mimc3_amd import api
    return api.wide_planes_max_radius(1) == R_MAX and hasattr(api.Context, "match_ncc_wide_planes")


assert _entry_exists()
SIX = fu.SIX
G4, G3CHIP, G3BOX, CLEAN, OUTSIDE, ONE_TILE = wu.G4, wu.G3CHIP, wu.G3BOX, wu.CLEAN, wu.OUTSIDE, wu.ONE_TILE
BOX_ONLY, CHIP_ONLY, BOTH = fu.BOX_ONLY, fu.CHIP_ONLY, fu.BOTH


# ---- the layout (match_wide_u16_kernel.hip wide_u16_layout): two tiles, two chip planes, the surface ----
def lds_bytes(ocw, R):
    cw = 2 * ocw + 1
    kw = cw + 31
    kcw = (cw + 15 + 63) // 64
    rdw, sw = 16 + 64 * kcw, (kw + 15) & ~15
    pw0 = max(rdw, sw)
    pw = pw0 if (pw0 // 16) & 1 else pw0 + 16
    ntr = (kw + 15) // 16
    cp = max((cw + 15 + 3) & ~3, 64 * kcw)
    chb = (16 + (cw + 1) * cp + 16 + 15) & ~15
    tb = (max((16 * ntr + 1) * pw, 1280) + 15) & ~15           # (one tile; the 1,280-byte bit plane of the candidate tail takes the first one's bytes)
    S = 2 * R + 1
    return kcw, 2 * tb + 2 * chb + ((S * 96 * 4 + 15) & ~15)


def max_radius(ocw):
    """the largest R <= 47 whose layout fits the 160 KB of a CU; 0 outside 1..80"""
    if not 1 <= ocw <= MAX_OCW:
        return 0
    return max((R for R in range(R_MIN, R_MAX + 1) if lds_bytes(ocw, R)[1] <= LDS_MAX), default=0)


def layout(ocw, R):
    """-> (K chunks per chip row, cell tiles per axis, threads per workgroup, dynamic LDS bytes), or None out of range"""
    if not (1 <= ocw <= MAX_OCW and R_MIN <= R <= max_radius(ocw)):
        return None
    kcw, lds = lds_bytes(ocw, R)
    return kcw, (2 * R + 1 + 31) // 32, 128, lds


# ---- the (ocw, R) table ----
RADII = wu.RADII                                        # 16, 23, 31 | 32, 47: see tests/wide_u8_common.py
def _drop(o):
    return max_radius(o - 1) - max_radius(o) if o >= 2 else 0


# the steps of the limit: the ocw at which it starts to fall (69, the first below 47: one per ocw from there) and at which it falls by
# more than that (73, where the tiles gain a 16-row group); both sides of each.  Between them the limit moves by one per ocw, the layout unchanged
STEPS = [o for o in range(2, MAX_OCW + 1) if _drop(o) > 0 and _drop(o) > _drop(o - 1)]
STEP_OCWS = sorted({o for s in STEPS for o in (s - 1, s)})
EDGE_OCWS = (1, 24, 25, 44, 45, 56, 57)                 # the KCW class edges, the single table query's limit
CASES = sorted({(o, r) for o in (7, 16) for r in RADII} | {(o, r) for o in EDGE_OCWS for r in (16, max_radius(o))} |
               {(o, max_radius(o)) for o in STEP_OCWS} | {(80, 16), (80, max_radius(80))})
# mode 1 at the six, against match_ncc_wide itself: ocw 7 and 16 at every R, ocw 32 at R 47, ocw 40 at R 39
SIX_CASES = [(o, r) for o in (7, 16) for r in RADII] + [(32, 47), (40, 39)]
OUTSIDE_CASES = [(o, r) for o, r in CASES if o not in SIX]
SATURATED = ((44, 16), (45, 16), (80, max_radius(80)))


# ---- fixtures ----
def _map(img8, kind):
    if kind in ("sat3", "sat63"):
        return np.array(top_of_class(img8, 4095, int(kind[3:])), np.float32)
    assert kind in ("dn12", "eighths", "mixed")
    return np.array(spread12(img8), np.float32)


def _fixture(ocw, R, kind, swap, with_shift):
    c, b0, b1, sh = fu.u8_case(ocw, R, "none", swap, with_shift)
    i0, i1 = _map(b0, kind), _map(b1, kind)
    assert i0.min() >= 1 and i1.min() >= 1 and max(i0.max(), i1.max()) <= 4095
    u, v, cu, cv = fu.geometry(c, sh, swap)
    chip_img, box_img = (i1, i0) if swap else (i0, i1)
    h = ocw + R
    # -4: the chip of point G4 copied to the border of its range, su = +R (the last, partial tile column), sv = 3: NCC = 1 there
    g = G4
    box_img[cv[g] + 3 - ocw:cv[g] + 3 + ocw + 1, cu[g] + R - ocw:cu[g] + R + ocw + 1] = chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
    # the placed nulls of full_chip_u8_common.u8_case
    g = BOX_ONLY[0]; box_img[cv[g] + h, cu[g] - 3] = 0              # the last box row
    g = BOX_ONLY[1]; box_img[cv[g] + 2, cu[g] + h] = 0              # the last box column
    g = CHIP_ONLY[0]; chip_img[v[g] - ocw, u[g]] = 0                # the first chip row
    g = CHIP_ONLY[1]; chip_img[v[g] + ocw, u[g] + ocw] = 0          # the last chip row (and column)
    g = BOTH[0]; chip_img[v[g], u[g] - 1] = 0; box_img[cv[g] + 1, cu[g]] = 0
    g = BOTH[1]; chip_img[v[g] - 1, u[g] - ocw] = 0; box_img[cv[g] - h, cu[g] + 1] = 0
    # -3 by the chip rule, -3 by the box rule (the chip stays as it is)
    g = G3CHIP; chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 0
    g = G3BOX; box_img[cv[g] - h:cv[g] + h + 1, cu[g] - h:cu[g] + h + 1] = 0
    # one null one column outside the box, in a row of the box: inside the last tile's reach, never read by the definition
    g = OUTSIDE; box_img[cv[g] + 1, cu[g] + h + 1] = 0
    # one null in the box that lies inside the window of tile (0, 0) and of no other (box pixel (3, 5): the other tiles start at 32)
    g = ONE_TILE; box_img[cv[g] - h + 5, cu[g] - h + 3] = 0
    if kind in ("eighths", "mixed"):
        i0 = i0 / np.float32(8)
    if kind == "eighths":
        i1 = i1 / np.float32(8)
    sgn = -1 if swap else 1
    off = np.ascontiguousarray(sgn * np.asarray(c.offset), np.int32)
    shift = None if sh is None else np.ascontiguousarray(sgn * np.asarray(sh), np.int32)
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    f = dict(c=c, i0=np.ascontiguousarray(i0, np.float32), i1=np.ascontiguousarray(i1, np.float32), xy=xy, off=off, shift=shift,
             case_shift=sh, ocw=ocw, R=R, swap=swap, kind=kind, what=f"ocw {ocw} R {R} {kind} swap {swap} shift {with_shift}")
    for a in (f["i0"], f["i1"], xy, off) + (() if shift is None else (shift,)):
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=4)
def fixture(ocw, R, kind="dn12", swap=False, with_shift=True):
    """-> dict(c, i0, i1, xy, off, shift, ocw, R, swap, kind, what): the arrays as the call takes them (swapped: offset and shift negated)"""
    return _fixture(ocw, R, kind, swap, with_shift)


def kinds(f):
    return wu.kinds(f)


def planes(f):
    """the pair as the integers q = 64 h + l that the u16 planes hold -> (q0, q1) int64"""
    s0 = 8 if f["kind"] in ("eighths", "mixed") else 1
    s1 = 8 if f["kind"] == "eighths" else 1
    q0, q1 = f["i0"].astype(np.float64) * s0, f["i1"].astype(np.float64) * s1
    assert np.array_equal(q0, np.rint(q0)) and np.array_equal(q1, np.rint(q1)) and max(q0.max(), q1.max()) < 4096
    return q0.astype(np.int64), q1.astype(np.int64)


def oracle_points(ocw):
    return wu.oracle_points(ocw)


@functools.lru_cache(maxsize=4)
def oracle(ocw, R, kind="dn12", swap=False, with_shift=True):
    """The CPU oracle on oracle_points(ocw) of the fixture -> (points, record, surfaces)"""
    f = fixture(ocw, R, kind, swap, with_shift)
    pts = oracle_points(ocw)
    rec, _, surf, _ = full_any(f["i0"], f["i1"], f["xy"][pts], f["off"], ocw, R, 0, shift=None if f["shift"] is None else f["shift"][pts], swap=swap)
    return pts, rec, surf


def all_fixtures():
    """(ocw, R, kind, swap, with_shift) of every placed-null fixture a GPU test uses"""
    out = {(o, r, "dn12", False, True) for o, r in CASES} | {(o, r, "dn12", False, True) for o, r in SIX_CASES}
    out |= {(16, 23, "dn12", True, True), (16, 23, "dn12", False, False), (10, 24, "dn12", True, True), (57, 16, "dn12", True, True),
            (16, 24, "dn12", False, True), (10, 24, "dn12", False, True), (24, 47, "dn12", False, True), (40, 45, "dn12", False, True)}
    out |= {(o, r, k, False, True) for o, r in SATURATED for k in ("sat3", "sat63")}
    out |= {(10, 24, "eighths", False, True), (10, 24, "mixed", False, True)}
    return sorted(out)


# ---- seams: wide_u8_common's periodic pairs on 12 bits, by_position=False so that they stay periodic ----
SEAM_OCW, SEAM_R, SEAM_PERIODS, PLATEAU_PERIOD, SEAM_PLATEAUS = wu.SEAM_OCW, wu.SEAM_R, wu.SEAM_PERIODS, wu.PLATEAU_PERIOD, wu.SEAM_PLATEAUS
maxima_cells = wu.maxima_cells


def seam_pair(pu, pv, plateau):
    """wide_u8_common.seam_pair with B spread over 12 bits (values up to 1920).  The plateau form is B + (B moved one row down) of the
    SPREAD B -- the flat top follows from the sum's linearity, which a spread of the sum would break -- at most 3840"""
    p0, p1, xy = wu.seam_pair(pu, pv, plateau)
    q0 = spread12(p0, by_position=False)
    q1 = q0 + spread12(p1 - p0, by_position=False) if plateau else spread12(p1, by_position=False)
    assert q1.max() < 4096
    return q0, np.ascontiguousarray(q1, np.float32), xy
