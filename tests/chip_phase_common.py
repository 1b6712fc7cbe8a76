"""Fixtures, call lists and the comparison of tests/test_chip_phases_cpu.py, tests/test_chip_phases.py and tests/test_chip_phases_acc.py:
the four run-time-ocw matrix-core searches -- match_ncc_full_chip_class (match_full_chip_u8_kernel.hip, "u8_mfma_chip"),
match_ncc_full_chip_planes (match_full_chip_u16_kernel.hip, "u16_mfma_chip"), match_ncc_wide_class beyond +-15 px
(match_wide_u8_kernel.hip, "u8_mfma_wide") and match_ncc_wide_planes beyond +-15 px (match_wide_u16_kernel.hip, "u16_mfma_wide") --
at every pixel phase of chip and window origin with every null class, and with one null at every position that a byte mask or a chunk
boundary can get wrong.  All four stage chip and window rows as aligned dwords and shift them by the phase of the row's first column
(csh = cu0 & 3, tsh = wu0 & 3; the wide kernels restage per tile at (wu0 + 32 tx) & 3, the u16 kernels shift by & 1); the last chip dword
is masked by LASTN = CW - 4 (CD - 1) (lastm in the wide u16 kernel); the masked forms build every null operand per byte in registers; the
wide kernels ask a table per tile (wn_t; the u32 null table in the u16 kernel) whether the tile's null corrections run at all.  The
accumulating (ACC) forms of all four -- stack_add_fused, stack_acc.h -- run over the same fixtures and calls (section 4).

The judge everywhere is the CPU oracle full_any_common.full_any (f64, the reference's operations), compared as
tests/test_wide_u8.py compares (`vs_oracle`): there is no tolerance.  For scaled pairs the oracle reads the integer images.

  1. `phase_fixture`: phase_common.fixture(plan "search") -- 64 points on odd spacings, all four chip phases, single-pixel nulls per
     point -- run over `phase_calls`: the four offsets in u with and without the a-priori shift, two of them swapped.  Beyond R 16 the
     fixture's boxes would overlap, and the grid is that of phase_common.geometry(ocw, reach=R).
  2. `sweep_fixture`: a null-free pair, a grid whose search boxes do not overlap, ONE planted null per point (`sweep_nulls`).
  3. phase_common.plane_end_points and phase_common.fractional on the fixtures of 1.
  4. `ACC_PHASE_CASES`, `ACC_SWEEP_CASES`: one stack_add_fused on a fresh stack per call, judged by `acc_judge` against
     stack_common.NumpyStack fed the oracle's surface."""
import collections
import functools
import types

import numpy as np

from conftest import assert_bits_equal
from full_any_common import full_any, tail_from_surface
from full_chip_u16_common import spread12
from mimc3_amd import synth
from phase_common import OFFSETS, SEARCH_R, fixture, phases, search_null_class, search_shifts
from stack_common import NumpyStack, refused_of
from u8_advance_common import box, null_table

# entry -> (the Context method, the path it must report)
ENTRIES = {"class": ("match_ncc_full_chip_class", "u8_mfma_chip"), "planes": ("match_ncc_full_chip_planes", "u16_mfma_chip"),
           "wide": ("match_ncc_wide_class", "u8_mfma_wide"), "wplanes": ("match_ncc_wide_planes", "u16_mfma_wide")}
WIDE = ("wide", "wplanes")                                # the entries whose kernels finish the cells in 32 x 32 tiles
U_OFFSETS = OFFSETS[:4]
NPEAKS = (0, 4)


def case_id(case):
    return "-".join(f"{k}{v}" if isinstance(v, int) else str(v) for k, v in zip(("", "", "ocw", "R"), case))


# ---- 1. every phase pair with every null class ------------------------------------------------------------------------------------------------
# ocw: both values of LASTN (CW mod 4 = 3 | 1), a chip row shorter than a dword pair (1, 2), KCW 1 | 2 | 3 on both sides of each edge
CHIP_OCWS = (1, 2, 10, 11, 24, 25, 45, 57, 80)
# (entry, kind, ocw, R)
PHASE_CASES = [("class", "u8", o, 7) for o in CHIP_OCWS] + [("class", "u8", 10, 15), ("class", "u8", 57, 15), ("class", "u8", 80, 1)]
PHASE_CASES += [("planes", k, o, 7) for o in CHIP_OCWS for k in ("12bit", "eighths")]
PHASE_CASES += [("planes", k, o, 15) for o in (10, 57) for k in ("12bit", "eighths")]
# the wide kernel: every chunk class at R 16 (S = 33: one cell column in the second tile); at small chips S = 47 (the second 16-column
# group), 63 | 65 (one column short of two tiles | a third tile of one column), 95 (3 x 3 one short); 2 x 2 tiles of a two-chunk chip row
WIDE_PHASES = [(o, 16) for o in (1, 10, 25, 45, 57, 80)] + [(7, 23), (7, 31), (7, 32), (3, 47), (25, 32)]
PHASE_CASES += [("wide", "u8", o, r) for o, r in WIDE_PHASES]
# the wide kernel on the u16 planes: the same (ocw, R), so that grid geometry and planted positions carry over
PHASE_CASES += [("wplanes", "12bit", o, r) for o, r in WIDE_PHASES] + [("wplanes", "eighths", 10, 16), ("wplanes", "eighths", 57, 16)]
# boxes at the end of the plane, and fractional coordinates
PLANE_END_CASES = [("class", "u8", 10, 7), ("class", "u8", 57, 15), ("planes", "12bit", 10, 7), ("planes", "12bit", 57, 15),
                   ("wide", "u8", 7, 32), ("wide", "u8", 25, 16), ("wplanes", "12bit", 7, 32), ("wplanes", "12bit", 25, 16)]
FRACTIONAL_CASES = [("class", "u8", 10, 7), ("planes", "12bit", 10, 7), ("planes", "eighths", 10, 7), ("wide", "u8", 10, 16),
                    ("wplanes", "12bit", 10, 16), ("wplanes", "eighths", 10, 16)]
FR_OFFSET = np.array([1, -1], np.int32)


def phase_fixture(case):
    """phase_common's search fixture of the case; beyond R 16 on the grid whose boxes of that radius do not overlap, below SEARCH_R with
    the window's null where a box of that radius holds it"""
    entry, kind, ocw, radius = case
    return fixture(ocw, kind, plan="search", reach=radius if radius > 16 or radius < SEARCH_R else None)


def phase_calls(f):
    """(offset, shift, swap): the four offsets in u with the a-priori shift and without, and the first of each swapped
    (tests/test_pixel_phases.py's search_calls over the offsets in u)"""
    prior, none = search_shifts(f)
    calls = [(np.asarray(o, np.int32), sh, False) for o in U_OFFSETS for sh in (prior, none)]
    return calls + [(-np.asarray(U_OFFSETS[1], np.int32), -prior, True), (-np.asarray(U_OFFSETS[2], np.int32), none, True)]


def call_cells(f, radius, calls):
    """the (chip phase, window phase, null class) cells that a list of calls reaches -> Counter; the key of
    phase_common.coverage(.., "search"), the null class counted in the images of each call's direction"""
    cells = collections.Counter()
    for offset, shift, swap in calls:
        p = phases(f.xy, offset, None, None, f.ocw, shift=shift, radius=radius)
        cells.update(zip(p["cph"].tolist(), p["wph"].tolist(), search_null_class(f, offset, shift, radius, swap=swap).tolist()))
    return cells


def integer_images(f):
    """the pair as the integers the kernels keep (eighths: pixel * 8): what the oracle reads"""
    s = np.float32(8) if f.kind == "eighths" else np.float32(1)
    return f.i0 * s, f.i1 * s


def oracle_search(f, radius, offset, shift, swap, xy=None, images=None):
    """the CPU oracle on the fixture's integer images (or on `images`) -> (record, surfaces)"""
    q0, q1 = integer_images(f) if images is None else images
    rec, _, surf, _ = full_any(q0, q1, f.xy if xy is None else xy, offset, f.ocw, radius, 0, shift=shift, swap=swap)
    return rec, surf


# the calls of phase_calls in three parts, so that no test waits for more than four runs of the oracle
PARTS = {"prior": (0, 2, 4, 6), "none": (1, 3, 5, 7), "swapped": (8, 9)}
# a part in halves, for the one case whose four oracle runs on the u16 pair take as long as the slowest test there was (the 8-bit case
# of the same ocw and R; measured on one MI355X host 2.50 s against 2.48 s): no new test is to take longer than that one
HALVES = {"prior-a": (0, 2), "prior-b": (4, 6), "none-a": (1, 3), "none-b": (5, 7), "swapped": (8, 9)}
HALVED_CASES = (("wplanes", "12bit", 80, 16),)
PHASE_PARTS = [(c, p) for c in PHASE_CASES for p in (HALVES if c in HALVED_CASES else PARTS)]


def part_calls(part):
    """the calls (indices into phase_calls) of a part of PARTS or HALVES"""
    return HALVES[part] if part in HALVES else PARTS[part]


def _phase_oracle(kind, ocw, radius, k):
    f = phase_fixture(("", kind, ocw, radius))
    return oracle_search(f, radius, *phase_calls(f)[k])


_recent_oracle = functools.lru_cache(maxsize=20)(_phase_oracle)
_kept_oracle = functools.lru_cache(maxsize=None)(_phase_oracle)


def phase_oracle(case, k):
    """(record, surfaces) of the oracle for call k of phase_calls, computed once per pair: an eighths pair holds the integers of the
    12-bit pair (tests/test_chip_phases_cpu.py asserts it), so the two share it.  The pairs of ACC_PHASE_CASES are kept for good (at
    most 1.1 MB per call), so that an accumulating case reads the oracle of its search case; every other pair leaves after 20 calls"""
    _, kind, ocw, radius = case
    kind = "12bit" if kind == "eighths" else kind
    return (_kept_oracle if (kind, ocw, radius) in ACC_PAIRS else _recent_oracle)(kind, ocw, radius, k)


# ---- the comparison: tests/test_wide_u8.py's vs_oracle ---------------------------------------------------------------------------------------
def same_surface(got, want, what):
    """finite cells bit for bit, a non-finite cell of the same kind"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what + ": finite cells differ"
    assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]), what + ": finite cells are not bit-equal"
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(got)], want[~fin & ~np.isnan(want)]), what + ": kinds"


def vs_oracle(got, o_rec, o_surf, shift, radius, npeaks, what):
    """(record, candidates, surfaces) of a call against the oracle's record and surfaces: the surface bit for bit, record and candidates
    the oracle's tail of the device surface AND of the oracle surface, the statuses -2, -3, -4 point for point"""
    rec, cand, surf = got
    st3 = o_rec[:, 2] == -3
    same_surface(surf, o_surf, what + ": surface vs the oracle")
    assert np.isnan(surf[st3]).all() and np.array_equal(rec[:, 2] == -3, st3), what + ": status -3 points"
    for name, s in (("device", surf), ("oracle", o_surf)):
        t_rec, t_cand = tail_from_surface(s, shift, radius, npeaks, refused=st3, device_snr_order=True)
        assert_bits_equal(rec, t_rec, f"{what}: record vs the tail of the {name} surface")
        if npeaks:
            assert_bits_equal(cand, t_cand, f"{what}: candidates vs the tail of the {name} surface")
    for k in (-2, -3, -4):
        assert np.array_equal(rec[:, 2] == k, o_rec[:, 2] == k), f"{what}: status {k}"


def search(ctx, entry, xy, offset, ocw, radius, npeaks, shift, swap, surface=True):
    """one call of the entry in mode 1 (the kernel under test at every chip size); the path is asserted, so no fallback stands in"""
    name, path = ENTRIES[entry]
    got = getattr(ctx, name)(xy, offset, ocw, radius, npeaks, shift=shift, swap=swap, mode=1, surface=surface)
    assert ctx.last_path() == path, f"{name}: path {ctx.last_path()}"
    return got


def check_call(ctx, entry, f, xy, radius, offset, shift, swap, o_rec, o_surf, what):
    """the entry at npeaks 0 and 4, with and without surfaces, against the oracle -> the results with surfaces, per npeaks"""
    out = []
    for npeaks in NPEAKS:
        tag = f"{what}, npeaks {npeaks}"
        got = search(ctx, entry, xy, offset, f.ocw, radius, npeaks, shift, swap)
        assert (got[1] is None) == (npeaks == 0), tag
        vs_oracle(got, o_rec, o_surf, shift, radius, npeaks, tag)
        bare = search(ctx, entry, xy, offset, f.ocw, radius, npeaks, shift, swap, surface=False)
        assert_bits_equal(bare[0], got[0], tag + ": record without surfaces")
        if npeaks:
            assert_bits_equal(bare[1], got[1], tag + ": candidates without surfaces")
        out.append(got)
    return out


# ---- 2. one null at every position that a mask or a chunk boundary can get wrong --------------------------------------------------------------
CHIP_SWEEPS = ((2, 7), (10, 7), (30, 7), (57, 7), (80, 7), (80, 15))
SWEEP_CASES = [(e, k, o, r) for e, k in (("class", "u8"), ("planes", "spread12")) for o, r in CHIP_SWEEPS]
SWEEP_CASES += [("wide", "u8", 7, 47), ("wide", "u8", 25, 32), ("wide", "u8", 57, 16)]
# the wide kernel on the u16 planes: the same three, and its radius limit at the largest chip (an LDS layout of 163,680 B)
SWEEP_CASES += [("wplanes", "spread12", 7, 47), ("wplanes", "spread12", 25, 32), ("wplanes", "spread12", 57, 16), ("wplanes", "spread12", 80, 27)]
SWEEP_DIMX = 8
SWEEP_OFFSET = np.array([1, -1], np.int32)


def tile_windows(ocw, radius):
    """one axis of the wide kernel's cell tiles: tile t finishes the cells 32 t .. 32 t + nc - 1, nc = min(32, S - 32 t), and its window
    -- the box pixels those cells read -- is [32 t, 32 t + CW + nc - 2] -> [(first, last) per tile]"""
    cw, S = 2 * ocw + 1, 2 * radius + 1
    return [(32 * t, 32 * t + cw + min(32, S - 32 * t) - 2) for t in range((S + 31) // 32)]


def tiles_holding(x, y, ocw, radius):
    """the tiles (tx, ty) whose window holds box pixel (x, y), by the intervals of tile_windows"""
    win = tile_windows(ocw, radius)
    return {(tx, ty) for tx, (a, b) in enumerate(win) if a <= x <= b for ty, (c, d) in enumerate(win) if c <= y <= d}


def tile_edge_nulls(ocw, radius):
    """For every tile (tx, ty) and either axis the four positions on both sides of the tile window's first and last pixel on that axis,
    those inside the box, the other coordinate 5 px inside the tile's window on the other axis (from its first pixel; in the last tile
    from its last, which no other tile's window holds) -> [(tx, ty, axis, inside, (x, y))]; inside: whether tile (tx, ty)'s window holds
    the pixel, which the coordinate on `axis` decides"""
    d2 = 2 * (ocw + radius) + 1
    win = tile_windows(ocw, radius)
    last = len(win) - 1
    mid = [min(a + 5, b) if t < last else max(b - 5, a) for t, (a, b) in enumerate(win)]
    out = []
    for ty in range(len(win)):
        for tx in range(len(win)):
            for axis, t, o in ((0, tx, mid[ty]), (1, ty, mid[tx])):
                a, b = win[t]
                for c, inside in ((a - 1, False), (a, True), (b, True), (b + 1, False)):
                    if 0 <= c < d2:
                        out.append((tx, ty, axis, inside, (c, o) if axis == 0 else (o, c)))
    return out


def sweep_nulls(entry, ocw, radius):
    """The planted nulls, one per point -> [(side, x, y)]: side "chip" (x, y chip pixel) or "box" (x, y pixel of the search box).
      chip: columns 0..4 (the four byte lanes of a dword, then the next dword), 63 | 64 | 65 and 127 | 128 (the K chunks of a chip row),
            CW - 2 | CW - 1 (the LASTN mask), those that exist; the rows cycle through 0, 1, ocw, CW - 1
      box:  columns 0..3, 15 | 16, 63 | 64, 79 | 80, D2 - 2 | D2 - 1 with the rows cycling through 0, 15 | 16, 63 | 64, 127 | 128 (the 64-row K
            chunks of the vertical sums), D2 - 1; then every one of those rows with the columns cycling
      wide: on each axis, for every tile, both sides of the tile window's first and last pixel: 32 t - 1, 32 t, 32 t + CW + nc - 2,
            32 t + CW + nc - 1 (tile_windows), those inside the box, the other coordinate cycling through the box's first, middle and last
            (both wide entries)
      wplanes: those four positions once more for every tile (tx, ty) of the grid, the other coordinate inside that tile's window
            (tile_edge_nulls): a query that is one column or row short in one tile only meets a null that only it can lose"""
    cw = 2 * ocw + 1
    d2 = cw + 2 * radius
    ccols = sorted(c for c in {0, 1, 2, 3, 4, 63, 64, 65, 127, 128, cw - 2, cw - 1} if 0 <= c < cw)
    crows = (0, 1, ocw, cw - 1)
    out = [("chip", c, crows[k % 4]) for k, c in enumerate(ccols)]
    bcols = sorted(c for c in {0, 1, 2, 3, 15, 16, 63, 64, 79, 80, d2 - 2, d2 - 1} if 0 <= c < d2)
    brows = sorted(r for r in {0, 15, 16, 63, 64, 127, 128, d2 - 1} if 0 <= r < d2)
    boxes = [(c, brows[k % len(brows)]) for k, c in enumerate(bcols)] + [(bcols[(5 * k + 3) % len(bcols)], r) for k, r in enumerate(brows)]
    if entry in WIDE:
        other = (0, d2 // 2, d2 - 1)
        k = 0
        for a, b in tile_windows(ocw, radius):
            for c in (a - 1, a, b, b + 1):
                if 0 <= c < d2:
                    boxes += [(c, other[k % 3]), (other[(k + 1) % 3], c)]
                    k += 1
    if entry == "wplanes":
        boxes += [t[-1] for t in tile_edge_nulls(ocw, radius)]
    seen = set()
    for xy in boxes:
        if xy not in seen:
            seen.add(xy)
            out.append(("box",) + xy)
    return out


@functools.lru_cache(maxsize=2)
def sweep_fixture(case):
    """-> namespace (i0, i1: the pair with every point's null planted; b0, b1: the null-free pair; xy, offset, shift, ocw, R, nulls:
    sweep_nulls, cu, cv: plane-free image position of every chip's pixel (0, 0), wu, wv: of every box's).  A texture without nulls, a
    grid of SWEEP_DIMX columns whose search boxes lie 2 (ocw + R) + 15 px apart (odd: the chip phase changes from column to column) under a
    shift of up to 3 px per point, which moves the window's phase against the chip's.  kind "spread12": full_chip_u16_common.spread12 of
    the same pair."""
    entry, kind, ocw, radius = case
    nulls = sweep_nulls(entry, ocw, radius)
    n = len(nulls)
    h = ocw + radius
    step, margin = 2 * h + 15, h + 12
    rows = (n + SWEEP_DIMX - 1) // SWEEP_DIMX
    H, W = 2 * margin + (rows - 1) * step + 1, 2 * margin + (SWEEP_DIMX - 1) * step + 1
    b0, b1 = synth.make_pair(H, W, (3, -2), 9500 + 100 * radius + ocw, noise_dn=2, bits=8, sigma=1.0)
    assert b0.min() >= 1 and b1.min() >= 1
    if kind == "spread12":
        b0, b1 = spread12(b0), spread12(b1)
    g = np.arange(n)
    u, v = margin + step * (g % SWEEP_DIMX), margin + step * (g // SWEEP_DIMX)
    xy = np.ascontiguousarray(np.stack([u * synth.MPP, -v * synth.MPP, u, v, 0 * u, 0 * u], axis=-1), np.float64)
    shift = np.ascontiguousarray(np.stack([(3 * g) % 7 - 3, (5 * g) % 7 - 3], axis=-1), np.int32)
    cu, cv = u - ocw, v - ocw
    wu, wv = u + int(SWEEP_OFFSET[0]) + shift[:, 0] - h, v + int(SWEEP_OFFSET[1]) + shift[:, 1] - h
    i0, i1 = b0.copy(), b1.copy()
    for k, (side, x, y) in enumerate(nulls):
        if side == "chip":
            i0[cv[k] + y, cu[k] + x] = 0
        else:
            i1[wv[k] + y, wu[k] + x] = 0
    for a in (i0, i1, b0, b1, xy, shift):
        a.setflags(write=False)
    return types.SimpleNamespace(i0=i0, i1=i1, b0=b0, b1=b1, xy=xy, offset=SWEEP_OFFSET, shift=shift, ocw=ocw, R=radius, nulls=nulls,
                                 cu=cu, cv=cv, wu=wu, wv=wv, kind=kind, entry=entry)


def sweep_moved(fx, d=1):
    """the pair with every point's null moved d pixels along u (the old place gets its pixel back) -> (i0, i1)"""
    i0, i1 = fx.b0.copy(), fx.b1.copy()
    for k, (side, x, y) in enumerate(fx.nulls):
        if side == "chip":
            i0[fx.cv[k] + y, fx.cu[k] + x + d] = 0
        else:
            i1[fx.wv[k] + y, fx.wu[k] + x + d] = 0
    return i0, i1


def null_counts(fx, i0=None, i1=None):
    """per point the nulls of its chip and of its search box, counted in the images -> two int arrays"""
    Sc, Sw = null_table(fx.i0 if i0 is None else i0), null_table(fx.i1 if i1 is None else i1)
    cw = 2 * fx.ocw + 1
    d2 = cw + 2 * fx.R
    return box(Sc, fx.cu, fx.cv, cw, cw), box(Sw, fx.wu, fx.wv, d2, d2)


def wn_tiles(fx, k, Sw=None):
    """The wn_t query of match_wide_u8_kernel.hip and match_wide_u16_kernel.hip restated: tile (tx, ty) runs its null corrections when the table of the window image
    counts a null in the rectangle at (wu0 + 32 tx, wv0 + 32 ty) of CW + ncx - 1 by CW + ncy - 1 pixels, ncx = min(32, S - 32 tx)
    -> the set of tiles of point k that do"""
    Sw = null_table(fx.i1) if Sw is None else Sw
    cw, S = 2 * fx.ocw + 1, 2 * fx.R + 1
    nt = (S + 31) // 32
    out = set()
    for ty in range(nt):
        for tx in range(nt):
            ncx, ncy = min(32, S - 32 * tx), min(32, S - 32 * ty)
            if box(Sw, fx.wu[k] + 32 * tx, fx.wv[k] + 32 * ty, cw + ncx - 1, cw + ncy - 1) > 0:
                out.add((tx, ty))
    return out


_kept_sweeps = {}


def wn_tiles_of_every_point(fx):
    """wn_tiles per point, over one table of the window image"""
    Sw = null_table(fx.i1)
    return [wn_tiles(fx, k, Sw) for k in range(len(fx.nulls))]


def sweep_oracle(fx, images=None):
    """(record, surfaces) of the oracle over the sweep fixture (or over `images` on its grid); those of ACC_SWEEP_CASES are kept"""
    case = (fx.entry, fx.kind, fx.ocw, fx.R)
    if images is None and case in _kept_sweeps:
        return _kept_sweeps[case]
    rec, _, surf, _ = full_any(*((fx.i0, fx.i1) if images is None else images), fx.xy, fx.offset, fx.ocw, fx.R, 0, shift=fx.shift)
    if images is None and case in ACC_SWEEP_CASES:
        rec.setflags(write=False)
        surf.setflags(write=False)
        _kept_sweeps[case] = rec, surf
    return rec, surf


# ---- 4. the accumulating forms: one stack_add_fused per fresh stack ------------------------------------------------------------------------------
# AccCfg (stack_acc.h) has 24 instantiations: KCW 1 | 2 | 3 (ocw 10 | 25 | 57 at these radii) x clean | masked x four kernels; every phase
# fixture holds clean and null points, every sweep point holds a null (all of them the masked form's)
ACC_PHASE_CASES = [("class", "u8", 10, 7), ("class", "u8", 25, 7), ("class", "u8", 57, 15)]
ACC_PHASE_CASES += [("planes", "12bit", 10, 7), ("planes", "12bit", 25, 7), ("planes", "12bit", 57, 7)]
ACC_PHASE_CASES += [("wide", "u8", 10, 16), ("wide", "u8", 25, 32), ("wide", "u8", 57, 16)]
ACC_PHASE_CASES += [("wplanes", "12bit", 10, 16), ("wplanes", "12bit", 25, 32), ("wplanes", "12bit", 57, 16)]
ACC_PARTS = ("prior", "swapped")
ACC_SWEEP_CASES = [("class", "u8", 10, 7), ("planes", "spread12", 10, 7), ("wide", "u8", 25, 32), ("wplanes", "spread12", 25, 32)]
ACC_PAIRS = {c[1:] for c in ACC_PHASE_CASES}
ACC_FINISHES = ((4, 1), (0, 2))                          # (npeaks, min_count): the single layer's mean; no cell holds two values


def acc_reference(o_rec, o_surf, radius, shift):
    """stack_common.NumpyStack fed ONE layer, the oracle's surface with refused_of(the oracle's record) -> its finishes at ACC_FINISHES"""
    ref = NumpyStack(o_surf.shape[0], radius, shift).add(o_surf, refused_of(o_rec))
    return [ref.finish(k, mc) for k, mc in ACC_FINISHES]


def acc_judge(got, o_rec, o_surf, radius, shift, what):
    """got: stack_finish(4, 1, surface=True) and stack_finish(0, 2, surface=True) of a stack that took one layer -> (record, candidates,
    layer counts, mean surface) each.  The mean surface is the oracle's bit for bit at finite cells and NaN elsewhere; the layer counts are
    NumpyStack's (1 per point the oracle does not refuse); record and candidates are NumpyStack.finish's bytes
    (tests/test_stack_fused.py); at min_count 2 every cell is NaN -- a cell that the clean AND the masked launch added holds two values
    whose mean is the single layer's, and shows only there"""
    want = acc_reference(o_rec, o_surf, radius, shift)
    (rec, cand, count, mean), (w_rec, w_cand, w_lay, w_mean) = got[0], want[0]
    fin = np.isfinite(o_surf)
    assert np.array_equal(np.isnan(mean), ~fin), what + ": the mean surface is NaN where the oracle's is not finite, and only there"
    assert np.array_equal(mean.view(np.uint32)[fin], o_surf.view(np.uint32)[fin]), what + ": mean surface vs the oracle, finite cells"
    assert_bits_equal(mean, w_mean, what + ": mean surface vs NumpyStack")
    assert count.dtype == np.uint16 and np.array_equal(count, w_lay), what + ": layer counts"
    assert np.array_equal(count, (o_rec[:, 2] != -3).astype(np.uint16)), what + ": one layer per point that is not refused"
    assert_bits_equal(rec, w_rec, what + ": record")
    assert_bits_equal(cand, w_cand, what + ": candidates")
    (rec2, cand2, count2, mean2), (w_rec2, _, w_lay2, w_mean2) = got[1], want[1]
    assert cand2 is None and np.isnan(mean2).all() and np.isnan(w_mean2).all(), what + ": min_count 2: a cell holds more than one value"
    assert np.array_equal(count2, w_lay2), what + ": min_count 2: layer counts"
    assert_bits_equal(rec2, w_rec2, what + ": min_count 2: record")


def acc_call(ctx, entry, xy, radius, offset, ocw, shift, swap):
    """one stack_add_fused on a fresh stack; the path is asserted, so no fallback stands in -> the finishes at ACC_FINISHES"""
    ctx.stack_begin_wide(xy.shape[0], radius, shift)
    ctx.stack_add_fused(xy, offset, ocw, swap=swap)
    assert ctx.last_path() == ENTRIES[entry][1], f"stack_add_fused: path {ctx.last_path()}"
    assert ctx.stack_info() == (xy.shape[0], radius, 1)
    return [ctx.stack_finish(k, mc, surface=True) for k, mc in ACC_FINISHES]
