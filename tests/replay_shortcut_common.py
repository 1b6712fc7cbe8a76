"""Test infrastructure of the exact replay's shortcut (match_mx_kernel.hip, "the shortcut"; match_px_kernel.hip's fast register form;
DESIGN 4.1.4): the rule restated in numpy beside the reference's sequential loop, the classes a point can fall into, and the small GPU
fixtures -- shared by tests/test_replay_shortcut_cpu.py and tests/test_replay_shortcut.py.

A point's climbs are the records of tests/test_mx_area_finish.py's speculative_climbs: per pivot (scan centres, moved flags, still
alive at the 16-scan cap), on the exact f32 surface, ignoring the visited state."""
import functools

import numpy as np

import test_mx_area_finish as af
import u8_advance_common as ac
from mimc3_amd import synth

SPEC_ROUNDS = af.SPEC_ROUNDS
OUTCOMES = ("short", "short_u", "fell_back", "no_pre")       # kReplayShort, kReplayShortU, kReplayFellBack, kReplayNoPre
CLASSES = ("w_first", "w_later_uncut", "cut_under_u_only", "cut_in_reality", "last_scan_moved", "capped", "equal_maxima", "no_scan")


def cells9(c):
    return {(c[0] + i, c[1] + j) for i in (-1, 0, 1) for j in (-1, 0, 1)}


def scan(val, c):
    """one scan centred on cell c = (cx, cy): (maximum of the nine cells, or None if no cell compares greater than -2; the move to the
    first cell attaining it in the reference's order :709-711, column outer), NaN cells never compare greater (:736)"""
    m, d = np.float32(-2.0), (0, 0)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            v = val[c[1] + j][c[0] + i]                     # (an array or its nested lists)
            if v > m:
                m, d = v, (i, j)
    return (m if m > np.float32(-2.0) else None), d


def maxima(val, climbs):
    """M_k: the running maximum of pivot k after all its recorded scans, -2 if no scan raised it"""
    out = []
    for centres, _, _ in climbs:
        m = np.float32(-2.0)
        for c in centres:
            s, _ = scan(val, c)
            if s is not None and s > m:
                m = s
        out.append(m)
    return out


def replay(centres, moves, seen):
    """the real climb of one pivot against the visited set `seen` (updated): scans performed -- a scan that does not move, or that
    meets no unvisited cell among its nine, is the last (the loop of af.stays_inside)"""
    t = 0
    for c, moved in zip(centres, moves):
        cells = cells9(c)
        fresh = not cells <= seen
        seen |= cells
        t += 1
        if not fresh or not moved:
            break
    return t


def end_cell(val, centres, moves, t):
    """where a pivot stands after its first t scans (a scan that does not move is the last one recorded)"""
    if t < len(centres):
        return centres[t]
    if not moves[-1]:
        return centres[-1]
    _, d = scan(val, centres[-1])                             # (the last recorded scan moved, to the first cell attaining its maximum)
    return (centres[-1][0] + d[0], centres[-1][1] + d[1])


def sequential(val, climbs, start):
    """the reference's loop over the pivots (:691-753) on recorded climbs: (peak cell, best, visited set, scans performed per pivot);
    `start` = the peak when no pivot raises the maximum.  Needs no lane alive at the cap (the records end there)."""
    seen, peak, best, T = set(), start, np.float32(-2.0), []
    for centres, moves, _ in climbs:
        t = replay(centres, moves, seen)
        T.append(t)
        m = np.float32(-2.0)
        for c in centres[:t]:
            s, _ = scan(val, c)
            if s is not None and s > m:
                m = s
        if t and m > best:
            peak, best = end_cell(val, centres, moves, t), m
    return peak, best, seen, T


def shortcut(val, climbs):
    """the rule: (outcome, w, peak cell, best) -- peak and best only for the two shortcut outcomes, where all nine fit cells count as
    visited"""
    if any(alive for _, _, alive in climbs):
        return "no_pre", None, None, None
    M = maxima(val, climbs)
    mstar = max(M) if M else np.float32(-2.0)
    if not mstar > np.float32(-2.0):
        return "no_pre", None, None, None
    w = [k for k, m in enumerate(M) if m == mstar][0]
    U = set()
    for centres, _, _ in climbs[:w]:
        for c in centres:
            U |= cells9(c)
    built = any(len(centres) > 0 for centres, _, _ in climbs[:w])
    centres, moves, _ = climbs[w]
    t = replay(centres, moves, set(U))
    if t == len(centres) and not moves[-1]:
        return ("short_u" if built else "short"), w, centres[-1], mstar
    return "fell_back", w, None, None


def classes(val, climbs, start):
    """the classes of CLASSES this point belongs to"""
    out = set()
    if any(alive for _, _, alive in climbs):
        return {"capped"}
    oc, w, _, _ = shortcut(val, climbs)
    M = maxima(val, climbs)
    if oc == "no_pre":
        return {"no_scan"}
    _, _, _, T = sequential(val, climbs, start)
    centres, moves, _ = climbs[w]
    if oc == "short":
        out.add("w_first")
    elif oc == "short_u":
        out.add("w_later_uncut")
    elif moves[-1] and T[w] == len(centres):
        out.add("last_scan_moved")
    elif T[w] == len(centres):
        out.add("cut_under_u_only")
    else:
        out.add("cut_in_reality")
    ends = {climbs[k][0][-1] for k, m in enumerate(M) if m == M[w] and climbs[k][0]}
    if len(ends) > 1:
        out.add("equal_maxima")
    return out


def check_point(val, climbs, start):
    """wherever the rule says "shortcut": peak cell, best and the nine visited bits equal the sequential result.  Returns the outcome."""
    oc, w, peak, best = shortcut(val, climbs)
    if oc in ("short", "short_u"):
        speak, sbest, seen, _ = sequential(val, climbs, start)
        assert peak == speak, (oc, w, peak, speak)
        assert np.float32(best).view(np.uint32) == np.float32(sbest).view(np.uint32), (oc, w, best, sbest)
        assert cells9(peak) <= seen, (oc, w, peak)
    return oc


# ---- GPU fixtures: images of at most 256 x 256 -------------------------------------------------------------------------------------------
def _small(ocw, seed, **kw):
    kw.setdefault("h", 256)
    kw.setdefault("w", 256)
    kw.setdefault("dimx", 6)
    kw.setdefault("dimy", 6)
    kw.setdefault("margin", ocw + 44)
    return ac.small(ocw, seed, **kw)


def _case(api, c, ocw):
    off, uv = ac.pivots(api, c, ocw)
    return c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw


def shifted_case(api, ocw):
    """a shifted pair whose peak lies on the corridor: the winner is the first pivot that scans"""
    return _case(api, _small(ocw, 9300 + ocw), ocw)


def noise_case(api, ocw):
    """two independent images: surfaces of independent noise with many local maxima"""
    c = _small(ocw, 9320 + ocw, speed=2300.0)
    d = _small(ocw, 9340 + ocw, speed=2300.0)
    return c.i0, d.i1, c.xyuvav, c.offset, *ac.pivots(api, c, ocw), ocw


def quantised_case(api, ocw):
    """a pair of two grey levels in blocks of 4 x 4 pixels: NCC values that tie exactly on different cells"""
    c = _small(ocw, 9360 + ocw, speed=2300.0)
    rng = np.random.default_rng(9360 + ocw)
    b = rng.integers(0, 2, (70, 70)).astype(np.float32)
    base = np.kron(b, np.ones((4, 4), np.float32)) * 100.0 + 60.0
    i0 = np.ascontiguousarray(base[8:264, 8:264])
    i1 = np.ascontiguousarray(base[8 - 2:264 - 2, 8 + 3:264 + 3])
    return i0, i1, c.xyuvav, c.offset, *ac.pivots(api, c, ocw), ocw


def nulls_case(api, ocw):
    """blobs of nulls in window and chip, and a constant patch in the chip image: chips without variance, whose every NCC is NaN, so
    that no scan raises a maximum"""
    c = _small(ocw, 9380 + ocw, null_frac=0.02)
    i0 = c.i0.copy()
    i0[:120, :170] = 90.0
    return i0, c.i1, c.xyuvav, c.offset, *ac.pivots(api, c, ocw), ocw


def far_case(api, ocw):
    """a smooth pair shifted far beyond the corridor's end: long climbs, some capped at 16 scans"""
    c = _small(ocw, 9400 + ocw, shift=(24, -20), speed=1500.0, sigma=9.0)
    return _case(api, c, ocw)


def off_corridor_case(api, ocw):
    """ac.off_corridor_case's geometry (a shift far off the corridor, long corridors, nulls) on a 256 x 256 pair"""
    c = ac.small(ocw, 8450 + ocw, null_frac=0.03 if ocw < 16 else 0.006, shift=(9, 7), angle_deg=45.0, speed=2900.0, h=256, w=256,
                 dimx=5, dimy=5, margin=ocw + 80)
    return _case(api, c, ocw)


CUT_POINTS = {7: (726, 1335, 1555), 16: (0, 337, 675)}


# "Cut under U but not in reality" does not happen with pivots along a line (none of 4,552 points searched): these points of the same dense
# grid carry hand-made pivot lists instead, found by a search over the recorded climbs of every cell of the point's pivot rectangle -- a
# first pivot a that climbs uncut, a second b whose real climb a's visited cells cut short, the winner w, one of whose scans lies
# inside a's scans and b's UNPERFORMED ones but not inside the performed ones, and the point's own last pivot (which sets the window)
CUT_U_POINTS = {7: ((308, ((4, -2), (5, -4), (4, -3), (18, -12))), (896, ((14, -9), (16, -10), (15, -7), (18, -12))),
                    (1211, ((2, -6), (1, -3), (1, -4), (19, -12))), (1358, ((17, -2), (19, -3), (18, -2), (19, -12)))),
                16: ((315, ((11, -10), (14, -7), (14, -9), (18, -12))), (539, ((0, -8), (4, -11), (3, -10), (19, -12))),
                     (581, ((0, -8), (1, -6), (0, -6), (19, -12))), (595, ((7, 0), (3, -4), (5, 0), (19, -12))))}


def cuts_case(api, ocw):
    """points of a dense grid on the independent-noise pair, picked by the rule in numpy: at ocw 7 the three of 1,600 whose winner's real
    climb is cut by the visited cells (no point of the 26 x 26 grid at ocw 16 is; on real images the class is that rare); and the
    points of CUT_U_POINTS with their hand-made pivot lists"""
    i0, i1 = noise_case(api, ocw)[:2]
    dim = 40 if ocw == 7 else 26
    c = _small(ocw, 9420 + ocw, speed=2300.0, dimx=dim, dimy=dim)
    off, uv = ac.pivots(api, c, ocw)
    keep = np.array(CUT_POINTS[ocw] + tuple(g for g, _ in CUT_U_POINTS[ocw]))
    uvs = [uv[off[i]:off[i + 1]] for i in CUT_POINTS[ocw]] + [np.array(p, np.int32) for _, p in CUT_U_POINTS[ocw]]
    for (g, p), i in zip(CUT_U_POINTS[ocw], keep[len(CUT_POINTS[ocw]):]):
        assert tuple(int(v) for v in uv[off[i + 1] - 1]) == p[-1], (ocw, g)      # (the window is the one of the point's own last pivot)
    off2 = np.zeros(len(keep) + 1, np.int64)
    off2[1:] = np.cumsum([len(p) for p in uvs])
    return i0, i1, np.ascontiguousarray(c.xyuvav[keep]), c.offset, off2, np.ascontiguousarray(np.concatenate(uvs), np.int32), ocw


FIXTURES = (("shifted", shifted_case), ("noise", noise_case), ("quantised", quantised_case), ("nulls", nulls_case),
            ("off_corridor", off_corridor_case), ("far", far_case), ("cuts", cuts_case))
OCWS = (7, 16)


@functools.lru_cache(maxsize=None)
def fixture(name, ocw):
    from mimc3_amd import api
    return dict(FIXTURES)[name](api, ocw)


@functools.lru_cache(maxsize=None)
def fixture_points(name, ocw):
    """per point of a fixture: (surface, climbs, start cell, classes, outcome of the rule)"""
    case = fixture(name, ocw)
    i0, i1, xy, offset, off, uv, _ = case
    out = []
    for g in range(len(xy)):
        val = af.surface(case, g)
        climbs = af.speculative_climbs(case, g, val)
        lu, lv = (int(v) for v in np.asarray(uv)[off[g + 1] - 1])
        start = (abs(lu) + 2, abs(lv) + 2)
        out.append((val, climbs, start, classes(val, climbs, start), shortcut(val, climbs)[0]))
    return out
