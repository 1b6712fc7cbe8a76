"""Fixtures of the exhaustive search beyond +-15 px on any pair at any chip half-width (mimc3_match_ncc_wide_chip,
match_wide_chip_kernel.hip) that the CPU and GPU tests share: the kernel's layout and the entry's dispatch table in Python terms, the
(tile, band) body choice of a point counted in numpy, the fixtures -- full_chip_u8_common's 12 points whose boxes do not overlap, mapped
to a pixel class FIRST and every null, -3 area and -4 chip copy planted afterwards -- and the judge that compares a result with the
oracle (tests/full_any_oracle.c through full_any_common.full_any / tail_from_surface)."""
import functools

import numpy as np

import full_chip_u8_common as fu
import wide_u8_common as wu
from full_any_common import full_any, surface_distance, tail_from_surface, to_float
from full_chip_common import band_shape, BAND_SHAPES, excluded
from full_chip_u16_common import spread12
from full_dn_common import to_dn16
from null_encoding_common import first_invalid_count

PATH, FLOAT_PATH, CHIP_PATH, U8_PATH, U16_PATH = "f32g_wide_chip", "f32g_wide", "f32g_chip", "u8_mfma_wide", "u16_mfma_wide"
MAX_OCW, R_MIN, R_MAX, CU_LDS = 80, 16, 47, 160 * 1024
STATIC_BYTES, HALF_BUDGET = 128, 79 * 1024
SIX = fu.SIX
BOX_ONLY, CHIP_ONLY, BOTH = fu.BOX_ONLY, fu.CHIP_ONLY, fu.BOTH
G4, G3CHIP, G3BOX, CLEAN, OUTSIDE, ONE_TILE = wu.G4, wu.G3CHIP, wu.G3BOX, wu.CLEAN, wu.OUTSIDE, wu.ONE_TILE
EXACT = ("u8", "dn12", "u16", "eighths")        # exact f64 sums: the oracle's surface bit for bit
SYMBOLS = ("mimc3_match_ncc_wide_chip", "mimc3_match_ncc_wide_chip_dev", "mimc3_wide_chip_max_radius", "mimc3_wide_chip_layout",
           "mimc3_wide_chip_path")


# ---- the layout (match_wide_chip_kernel.hip wide_chip_layout) ----
def layout_full(ocw, R):
    cw = 2 * ocw + 1
    cwp = (cw + 3) & ~3
    bw = cwp + 32
    pb = bw if (bw // 4) & 1 else bw + 4
    S = 2 * R + 1
    surf = (S * 96 * 4 + 15) & ~15
    row, fixed = 4 * (pb + cwp), 4 * 31 * pb
    two = fixed + cw * row + surf <= HALF_BUDGET
    br = min(((HALF_BUDGET if two else CU_LDS - STATIC_BYTES) - surf - fixed) // row, cw)
    off_chip = 4 * (br + 31) * pb
    lds = ((off_chip + 4 * br * cwp + 15) & ~15) + surf
    return dict(CW=cw, CWP=cwp, PB=pb, KW=cw + 31, S=S, NTX=(S + 31) // 32, BR=br, NB=-(-cw // br) if br > 0 else 0, lds=lds,
                wgs=min(CU_LDS // (lds + STATIC_BYTES), 8))


def layout(ocw, R):
    """-> (tiles per axis, band rows, bands, workgroups per CU, dynamic LDS bytes), or None out of range"""
    if not (1 <= ocw <= MAX_OCW and R_MIN <= R <= R_MAX):
        return None
    L = layout_full(ocw, R)
    return L["NTX"], L["BR"], L["NB"], L["wgs"], L["lds"]


def band_shape_cases(query):
    """For each of full_chip_common.BAND_SHAPES one (ocw, R) in the entry's own range, from the layout `query` (the library's on the GPU
    side): the largest R that has a chip size of that shape, and at that R the largest such ocw"""
    found = {}
    for R in range(R_MAX, R_MIN - 1, -1):
        for ocw in range(MAX_OCW, 0, -1):
            s = band_shape(2 * ocw + 1, query(ocw, R)[1])
            if s and s not in found:
                found[s] = (ocw, R)
    return found


# ---- the dispatch table (include/mimc3_hip.h) ----
WIDE_MAX = {7: 47, 15: 47, 16: 47, 30: 47, 32: 47, 40: 39}     # mimc3_wide_max_radius at the six


def path(cls, ocw, R, mode, planes_max):
    """the table as a last_path number; planes_max(ocw) = mimc3_wide_planes_max_radius"""
    if not (0 <= cls <= 3 and 1 <= ocw <= MAX_OCW and 1 <= R <= R_MAX and mode in (0, 1)):
        return -1
    if R <= 15:
        if mode == 1:
            return 11
        return (6, 7, 8, 9)[cls] if ocw in SIX else (12, 13, 11, 11)[cls]
    if mode == 1:
        return 16
    if cls == 0:
        return 14
    if cls == 1:
        return 15 if R <= planes_max(ocw) else 16
    return 10 if ocw in SIX and R <= WIDE_MAX[ocw] else 16


# ---- fixtures ----
KINDS = ("u8", "dn12", "u16", "float", "wide", "eighths")


def _amplitude(shape):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return np.power(10.0, 3.0 * np.sin(2 * np.pi * (xx + 0.6 * yy) / 160.0)).astype(np.float32)


def _map(img8, kind, seed):
    if kind == "u8":
        return np.array(img8, np.float32)
    if kind == "dn12":
        return np.array(spread12(img8), np.float32)
    if kind == "u16":
        return np.array(to_dn16(img8, seed), np.float32)
    if kind == "eighths":
        return np.array(to_dn16(img8, seed) / np.float32(8), np.float32)
    f = to_float(img8, seed)
    return (f * _amplitude(f.shape)).astype(np.float32) if kind == "wide" else np.array(f, np.float32)


def _fixture(ocw, R, kind, swap, with_shift, enc, status):
    c, b0, b1, sh = fu.u8_case(ocw, R, "none", swap, with_shift)
    i0, i1 = _map(b0, kind, 1000 + ocw), _map(b1, kind, 2000 + ocw)
    assert i0.min() > 0 and i1.min() > 0
    u, v, cu, cv = fu.geometry(c, sh, swap)
    chip_img, box_img = (i1, i0) if swap else (i0, i1)
    h = ocw + R
    D = 2 * h + 1
    # -4: the chip of point G4 copied to the border of its range, su = +R (the last, partial tile column), sv = 3: NCC = 1 there
    g = G4
    box_img[cv[g] + 3 - ocw:cv[g] + 3 + ocw + 1, cu[g] + R - ocw:cu[g] + R + ocw + 1] = chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
    g = BOX_ONLY[0]; box_img[cv[g] + h, cu[g] - 3] = 0              # the last box row only: the last band of the last tile row
    g = BOX_ONLY[1]; box_img[cv[g] + 2, cu[g] + h] = 0              # the last box column only: the last tile column
    g = CHIP_ONLY[0]; chip_img[v[g] - ocw, u[g]] = 0                # the first chip row only: the first band of every tile
    g = CHIP_ONLY[1]; chip_img[v[g] + ocw, u[g] + ocw] = 0          # the last chip row (and column)
    g = BOTH[0]; chip_img[v[g], u[g] - 1] = 0; box_img[cv[g] + 1, cu[g]] = 0
    g = BOTH[1]; chip_img[v[g] - 1, u[g] - ocw] = 0; box_img[cv[g] - h, cu[g] + 1] = 0
    box = box_img[cv[G3BOX] - h:cv[G3BOX] + h + 1, cu[G3BOX] - h:cu[G3BOX] + h + 1]
    if status:
        # the box rule with the first null count beyond 80 %; a share of 60 % that must be searched (a count taken once per tile would
        # see every pixel of it up to nine times); a flat chip (-2: no finite cell)
        rng = np.random.default_rng(ocw + R)
        box[np.unravel_index(rng.choice(D * D, first_invalid_count(D * D), replace=False), box.shape)] = 0
        g = CLEAN
        b9 = box_img[cv[g] - h:cv[g] + h + 1, cu[g] - h:cu[g] + h + 1]
        b9[np.unravel_index(rng.choice(D * D, int(0.6 * D * D), replace=False), b9.shape)] = 0
        g = ONE_TILE
        chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 9 * 256 + 77      # (its square is exact in f32: the variance is 0)
    else:
        # one null in the box that lies inside the window of tile (0, 0) and of no other (box pixel (3, 5): the other tiles start at 32)
        g = ONE_TILE; box_img[cv[g] - h + 5, cu[g] - h + 3] = 0
    # one null one column outside the box, in a row of the box: inside the last tile's overhang, never read by the definition
    g = OUTSIDE; box_img[cv[g] + 1, cu[g] + h + 1] = 0
    if enc == "nan_zero":
        i0[i0 == 0] = np.nan
    elif enc == "m9999_nan":
        i0[i0 == 0] = -9999.0
        i1[i1 == 0] = np.nan
    else:
        assert enc == "zero"
    # -3 by the chip rule and by the box rule: pixels below MIN_DN whatever the null encoding (a NaN is not counted), so planted last
    g = G3CHIP; chip_img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 0
    if status:
        box[np.isnan(box)] = 0
    else:
        box[:] = 0
    sgn = -1 if swap else 1
    off = np.ascontiguousarray(sgn * np.asarray(c.offset), np.int32)
    shift = None if sh is None else np.ascontiguousarray(sgn * np.asarray(sh), np.int32)
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    f = dict(i0=np.ascontiguousarray(i0, np.float32), i1=np.ascontiguousarray(i1, np.float32), xy=xy, off=off, shift=shift, ocw=ocw, R=R,
             swap=swap, kind=kind, exact=kind in EXACT, status=status, geo=(u, v, cu, cv),
             what=f"ocw {ocw} R {R} {kind} {enc} swap {swap} shift {with_shift}" + (" status" if status else ""))
    for a in (f["i0"], f["i1"], xy, off) + (() if shift is None else (shift,)):
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=6)
def fixture(ocw, R, kind="u16", swap=False, with_shift=True, enc="zero", status=False):
    """-> dict(i0, i1, xy, off, shift, ocw, R, swap, kind, exact, what, ...): the arrays as the call takes them (swapped: offset and shift
    negated), shared and read-only.  status: the status fixture (the box rule at its limit, a 60 % box, a flat chip)"""
    return _fixture(ocw, R, kind, swap, with_shift, enc, status)


# the points a fixture is run on: all 12 up to ocw 44, 8 from there, 4 at ocw 80 (the oracle takes 0.7 s a point at ocw 80, R 47)
def points(ocw):
    if ocw >= 70:
        return (BOX_ONLY[1], CHIP_ONLY[0], G4, G3CHIP)
    return tuple(range(12)) if ocw < 45 else wu.ORACLE_POINTS_BIG


def sub(f, pts):
    """the call's arrays restricted to the points pts -> (xy, shift)"""
    pts = list(pts)
    return np.ascontiguousarray(f["xy"][pts]), None if f["shift"] is None else np.ascontiguousarray(f["shift"][pts])


@functools.lru_cache(maxsize=6)
def oracle(ocw, R, kind="u16", swap=False, with_shift=True, enc="zero", status=False):
    """The CPU oracle on points(ocw) of the fixture, computed once per process -> (points, record, surfaces)"""
    f = fixture(ocw, R, kind, swap, with_shift, enc, status)
    pts = points(ocw)
    xy, sh = sub(f, pts)
    rec, _, surf, _ = full_any(f["i0"], f["i1"], xy, f["off"], ocw, R, 0, shift=sh, swap=swap)
    rec.setflags(write=False); surf.setflags(write=False)
    return pts, rec, surf


def tile_band_classes(f, g, query=layout):
    """The body of every (tile, band) of point g as the kernel chooses it -> bool[NTX][NTX][bands] (ty, tx, band), True = masked: an
    excluded pixel among the band's chip rows, or among the box pixels of the band's window -- rows 32 ty + r0 .. + h + 30, columns
    32 tx .. + CW + 30 -- that lie INSIDE the box.  (The fixtures' boxes lie inside the image.)"""
    ocw, R = f["ocw"], f["R"]
    ntx, br, nb = query(ocw, R)[:3]
    u, v, cu, cv = (a[g] for a in f["geo"])
    chip_img, box_img = (f["i1"], f["i0"]) if f["swap"] else (f["i0"], f["i1"])
    h, cw = ocw + R, 2 * ocw + 1
    chip = excluded(chip_img[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1])
    box = excluded(box_img[cv - h:cv + h + 1, cu - h:cu + h + 1])
    assert box.shape == (2 * h + 1, 2 * h + 1)
    out = np.zeros((ntx, ntx, nb), bool)
    for ty in range(ntx):
        for tx in range(ntx):
            for b in range(nb):
                r0 = b * br
                hh = min(br, cw - r0)
                out[ty, tx, b] = chip[r0:r0 + hh].any() or box[32 * ty + r0:32 * ty + r0 + hh + 31, 32 * tx:32 * tx + cw + 31].any()
    return out


# ---- the judge ----
def same_surface(got, want, what):
    """finite cells bit for bit, a non-finite cell of the same kind"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what + ": finite cells differ"
    assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]), what + ": finite cells are not bit-equal"
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(got)], want[~fin & ~np.isnan(want)]), what + ": kinds"


def judge(got, o_rec, o_surf, shift, radius, npeaks, exact, what):
    """record, candidates and surface of a call (on the oracle's points) against the oracle's record and surfaces: the surface bit for
    bit on an exact pair, within 1 f32 ulp on a float pair; the statuses; record and candidates equal the tail of the DEVICE surface bit
    for bit on every pair"""
    from conftest import assert_bits_equal
    rec, cand, surf = got
    st3 = o_rec[:, 2] == -3
    assert np.array_equal(rec[:, 2] == -3, st3), what + ": status -3"
    assert np.isnan(surf[st3]).all(), what + ": a refused point's surface is all NaN"
    if exact:
        same_surface(surf, o_surf, what + ": surface vs the oracle")
    else:
        share, worst = surface_distance(surf, o_surf, what)
        print(f"{what}: {share:.4f} of the finite cells differ, at most {worst} ulp")
        assert worst <= 1, f"{what}: a finite cell is {worst} ulp from the oracle"
    t_rec, t_cand = tail_from_surface(surf, shift, radius, npeaks, refused=st3, device_snr_order=True)
    assert_bits_equal(rec, t_rec, what + ": record vs the tail of the device surface")
    if npeaks:
        assert_bits_equal(cand, t_cand, what + ": candidates vs the tail of the device surface")
    else:
        assert cand is None
    if exact:
        for k in (-2, -4):
            assert np.array_equal(rec[:, 2] == k, o_rec[:, 2] == k), f"{what}: status {k}"


# ---- every standard fixture a GPU test of tests/test_wide_chip.py runs in mode 1: (ocw, R, kind, swap, with_shift, enc, status) ----
TILE_EDGES = [(10, 16, "u16", False, True, "zero", False), (10, 31, "u16", False, False, "zero", False),
              (10, 32, "u16", True, True, "zero", False), (10, 47, "u16", False, True, "zero", False)]
BODIES = [(10, 24, "float", False, True, "m9999_nan", False), (10, 24, "wide", False, True, "zero", False),
          (10, 24, "wide", False, True, "nan_zero", False)]
STATUS = (10, 32, "u16", False, True, "zero", True)
FIXED_SIZES = [(80, 16), (80, 47), (1, 16)]


def band_fixtures(query=layout):
    # (a full last band does not occur in this layout: a chip has an odd number of rows and a multi-band chip's band at least 71 of
    #  them -- tests/test_wide_chip_cpu.py asserts it; every shape that does occur is taken)
    found = band_shape_cases(query)
    sizes = [found[s] for s in BAND_SHAPES if s in found] + FIXED_SIZES
    return [(o, r, "u16", False, True, "zero", False) for o, r in sizes]


def all_fixtures(query=layout):
    return TILE_EDGES + BODIES + [STATUS] + band_fixtures(query) + [(16, 24, "u16", False, True, "zero", False), (40, 39, "u16", False, True, "zero", False),
                                                                      (16, 24, "u8", False, True, "zero", False), (40, 39, "u8", False, True, "zero", False)]
