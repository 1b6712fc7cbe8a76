#!/usr/bin/env python3
"""Generate tests/golden/ncc_edge_ocw*.npz: NCC cells at f32 rounding boundaries (see tests/ncc_edge_common.py for the format).

    python tests/golden/make_ncc_edge_fixtures.py [--jobs N]

Per chip size: a smooth 8-bit texture, its copy moved by OFFSET plus a little noise, points on a grid far enough apart that no point's
cells read another point's rewritten pixels.  For each point a target cell (the peak (0, 0) or one of its 8 neighbours) is pushed to a
wanted distance d from an f32 rounding midpoint by rewriting three window pixels under it (tests/golden/ncc_edge_search.c, a brute
force over the pixels' values).  A hit is kept only when the port oracle's DLC match and the exhaustive-search oracle
both still put the peak on (0, 0); otherwise the search resumes after it.  Deterministic: the same arrays on every run.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mimc3_amd import synth  # noqa: E402
from ncc_edge_common import NEIGHBOURS, T_D, midpoint_distance, qd, cell_sums, surface  # noqa: E402

SRC = os.path.join(HERE, "ncc_edge_search.c")
LIB = os.path.join(ROOT, "tests", "_build", "libncc_edge_search.so")
FLAGS = ["-O3", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-fPIC", "-shared", "-std=gnu11", "-Wall"]
OFFSET = (2, -1)
RADIUS = 4                        # the exhaustive search's radius; climbs reach (+-4, +-1) at most, cells +-5
DELTA = 255                       # a rewritten pixel takes any value 1..255
NPOS = 12                         # candidate pixels per target cell (C(12, 3) triples of 255^3 candidates)
MAX_CAND = 3_000_000_000
# chip size -> (grid columns, grid rows, texture seed)
PLAN = {7: (12, 9, 7001), 15: (4, 4, 7015), 16: (7, 6, 7016), 30: (3, 2, 7030), 32: (3, 2, 7032), 40: (3, 3, 7040)}
# wanted d, cycled over a chip size's points: (lo, hi); negative ranges ask for the other rounding direction
NEAR = [(1, 4), (-4, -1)]
CLASSES = NEAR * 5 + [(5, 64), (-64, -5), (8192 - 16, 8192 + 16), (-8192 - 16, -8192 + 16), (16384 - 16, 16384 + 16),
                      (-16384 - 16, -16384 + 16)] + NEAR * 6
ZERO_EVERY = 17                   # every 17th point asks for d = 0 first (an exact midpoint), then falls back to 1 <= |d| <= 4


def _lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        tmp = "%s.%d" % (LIB, os.getpid())
        subprocess.check_call(["gcc", *FLAGS, "-o", tmp, SRC, "-lm"])
        os.replace(tmp, LIB)
    lib = C.CDLL(LIB)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.edge_search.argtypes = [i32p, i32p, C.c_int, i32p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64,
                                np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")]
    lib.edge_search.restype = C.c_int
    return lib


def layout(ocw):
    nx, ny, seed = PLAN[ocw]
    sp = 2 * ocw + 2 * RADIUS + 2
    m = ocw + RADIUS + 8
    H, W = 2 * m + (ny - 1) * sp + 1, 2 * m + (nx - 1) * sp + 1
    n = nx * ny
    xy = np.zeros((n, 6))
    for g in range(n):
        xy[g, :4] = (g % nx, g // nx, m + (g % nx) * sp, m + (g // nx) * sp)
    return H, W, seed, xy


def point_plan(g):
    """(role, form, wanted d ranges, pivots) of point g."""
    form = g % 3
    climb = g % 12 == 0
    role = 0 if (climb or (g // 3) % 2 == 0) else 1 + (g // 6) % 8
    lo_hi = CLASSES[g % len(CLASSES)]
    want = [(0, 0), NEAR[g % 2]] if g % ZERO_EVERY == 5 else [lo_hi]
    want.append((-want[-1][1], -want[-1][0]))                  # the other rounding direction if a range has no cell
    if climb:
        piv = [(4, 1)] if (g // 12) % 2 == 0 else [(-1, -4)]    # reached after 5 scans
    else:
        piv = [(0, 0), (1, 0)] if g % 2 == 0 else [(0, 0), (0, -1)]
    return role, form, want, piv


def base_pair(ocw):
    H, W, seed, xy = layout(ocw)
    rng = np.random.Generator(np.random.PCG64(seed))
    i0 = synth.texture(H, W, seed, sigma=2.0).astype(np.int32)
    i1 = np.roll(i0, (OFFSET[1], OFFSET[0]), axis=(0, 1)) + rng.integers(-6, 7, size=(H, W))
    i1 = np.clip(i1, 1, 255).astype(np.int32)
    for g in range(xy.shape[0]):
        role, form, _, _ = point_plan(g)
        su, sv = (0, 0) if role == 0 else NEIGHBOURS[role - 1]
        u0, v0 = int(xy[g, 2]), int(xy[g, 3])
        if form == 1:          # two null window pixels inside the target cell's box
            uc, vc = u0 + OFFSET[0] + su, v0 + OFFSET[1] + sv
            i1[vc - ocw + 1, uc - ocw + 2] = 0
            i1[vc + ocw - 2, uc + 1] = 0
        elif form == 2:        # two null chip pixels
            i0[v0 - ocw + 2, u0 - ocw + 1] = 0
            i0[v0 + 1, u0 + ocw - 2] = 0
    return i0, i1, xy


def _box(i0, i1, xy, ocw, g, su, sv):
    u0, v0 = int(xy[g, 2]), int(xy[g, 3])
    uc, vc = u0 + OFFSET[0] + su, v0 + OFFSET[1] + sv
    a = np.ascontiguousarray(i0[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1], np.int32).ravel()
    b = np.ascontiguousarray(i1[vc - ocw:vc + ocw + 1, uc - ocw:uc + ocw + 1], np.int32).ravel()
    return a, b, uc - ocw, vc - ocw


def search(job):
    """One target cell, one wanted range, `skip` hits passed over -> (g, edits [(y, x, value)] or None, d)."""
    ocw, g, lo_hi, skip = job
    i0, i1, xy = base_pair(ocw)
    role, _, _, _ = point_plan(g)
    su, sv = (0, 0) if role == 0 else NEIGHBOURS[role - 1]
    a, b, x0, y0 = _box(i0, i1, xy, ocw, g, su, sv)
    cw = 2 * ocw + 1
    ok = np.flatnonzero((a != 0) & (b != 0))
    rng = np.random.Generator(np.random.PCG64(1000 * ocw + g))
    pos = np.ascontiguousarray(np.sort(rng.choice(ok, min(NPOS, ok.size), replace=False)), np.int32)
    out = np.zeros(7, np.int64)
    lo, hi = lo_hi
    hit = _lib().edge_search(a, b, cw * cw, pos, pos.size, DELTA, lo, hi, 0, skip, MAX_CAND, out)
    if not hit:
        return g, None, None
    edits = [(y0 + int(p) // cw, x0 + int(p) % cw, int(v)) for p, v in zip(out[:3], out[3:6])]
    return g, edits, int(out[6])


def accept(i0, i1, xy, ocw, g, piv, orc, full_search):
    """The peak stays on (0, 0): the strict maximum of the (2R + 1)^2 box, the DLC port oracle's and the exhaustive search's peak."""
    S = 2 * RADIUS + 1
    surf = surface(i0, i1, xy, OFFSET, ocw, g, RADIUS)
    f32 = surf.astype(np.float32)
    kc = RADIUS * S + RADIUS
    flat = f32.ravel()
    if not (flat[kc] == flat.max() and (flat == flat.max()).sum() == 1):
        return False
    pts = xy[g:g + 1]
    off = np.array([0, len(piv)], np.int64)
    uv = np.array(piv, np.int32)
    out = orc.match(i0.astype(np.float32), i1.astype(np.float32), pts, OFFSET, off, uv, ocw)
    if out[0, 2] != flat[kc] or abs(out[0, 0]) >= 1 or abs(out[0, 1]) >= 1:
        return False
    _, pk = full_search(i0.astype(np.float32), i1.astype(np.float32), pts, OFFSET, ocw, RADIUS, with_peak=True)
    return int(pk[0]) == kc


def build(ocw, pool):
    from oracle.oracle import Oracle
    from full_search_common import full_search
    orc = Oracle("port")
    i0, i1, xy = base_pair(ocw)
    n = xy.shape[0]
    plans = [point_plan(g) for g in range(n)]
    state = {g: [0, 0] for g in range(n)}              # g -> [index into the wanted ranges, hits skipped]
    done = {}
    while len(done) < n:
        jobs = [(ocw, g, plans[g][2][state[g][0]], state[g][1]) for g in range(n) if g not in done]
        for g, edits, d in pool.map(search, jobs, chunksize=1):
            if edits is None:
                state[g][0] += 1
                state[g][1] = 0
                if state[g][0] == len(plans[g][2]):
                    raise RuntimeError(f"ocw {ocw} point {g}: no cell in {plans[g][2]}")
                continue
            t0, t1 = i0.copy(), i1.copy()
            for y, x, v in edits:
                t1[y, x] = v
            if accept(t0, t1, xy, ocw, g, plans[g][3], orc, full_search):
                done[g] = (edits, d)
            else:
                state[g][1] += 1
    for g in range(n):
        for y, x, v in done[g][0]:
            i1[y, x] = v
    targets, piv_uv, piv_off = [], [], [0]
    for g in range(n):
        role, form, _, piv = plans[g]
        su, sv = (0, 0) if role == 0 else NEIGHBOURS[role - 1]
        d = midpoint_distance(qd(cell_sums(i0, i1, xy, OFFSET, ocw, g, su, sv)))
        assert d == done[g][1], (ocw, g, d, done[g][1])
        assert accept(i0, i1, xy, ocw, g, piv, orc, full_search), (ocw, g)
        targets.append((g, su, sv, role, form, d))
        piv_uv += piv
        piv_off.append(len(piv_uv))
    assert i0.min() >= 0 and i0.max() <= 255 and i1.min() >= 0 and i1.max() <= 255
    return dict(i0=i0.astype(np.uint8), i1=i1.astype(np.uint8), xyuvav=xy, offset=np.array(OFFSET, np.int32), ocw=np.int32(ocw),
                radius=np.int32(RADIUS), piv_off=np.array(piv_off, np.int64), piv_uv=np.array(piv_uv, np.int32).reshape(-1, 2),
                targets=np.array(targets, np.int64))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--ocw", type=int, nargs="*", default=sorted(PLAN))
    a = ap.parse_args()
    _lib()
    with Pool(a.jobs) as pool:
        for ocw in a.ocw:
            f = build(ocw, pool)
            path = os.path.join(HERE, "ncc_edge_ocw%02d.npz" % ocw)
            np.savez_compressed(path, **f)
            d = f["targets"][:, T_D]
            print(f"{os.path.basename(path)}: {len(d)} cells, {int(((np.abs(d) >= 1) & (np.abs(d) <= 4)).sum())} at 1 <= |d| <= 4, "
                  f"{int((d == 0).sum())} at d = 0, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
