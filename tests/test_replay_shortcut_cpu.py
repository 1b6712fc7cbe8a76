"""The exact replay's shortcut, without a GPU: the rule restated in numpy (tests/replay_shortcut_common.py) beside the
reference's sequential loop over the pivots -- the loop of tests/test_mx_area_finish.py's stays_inside, on the climbs of its
speculative_climbs.  Wherever the rule says "shortcut", the peak cell, the best value and the nine visited bits of the fit must be the
sequential result's.  On 21,000 seeded random surfaces of 12 x 12 to 31 x 31 cells (smooth bumps with noise, independent noise with
many local maxima, surfaces quantised to a few values so that maxima tie exactly; pivot lines in all eight directions), and on every
point of the GPU fixtures of tests/test_replay_shortcut.py, which are qualified here: each class of points the rule distinguishes must
hold at least five of them."""
import collections
import functools

import numpy as np
import pytest

import replay_shortcut_common as rc
import test_mx_area_finish as af

DIRS8 = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1))
N_SURFACES = 21000
OCW = 7             # (the surfaces are made directly: the chip size only places the cells in the window)


def random_point(rng, i):
    """(surface, climbs, start cell) of one random point"""
    S = int(rng.integers(12, 32))
    sx, sy = DIRS8[i % 8]
    a = int(rng.integers(2, (S - 6) // 2 + 1))
    b = int(rng.integers(1, a + 1))
    lu, lv = sx * a, sy * (b if sx else a)
    kind = (i // 8) % 3
    val = rng.uniform(-0.3, 0.3, (S, S))
    if kind == 0:                                             # a bump somewhere in the grid, with noise
        cy, cx = rng.uniform(1, S - 2, 2)
        yy, xx = np.mgrid[:S, :S]
        val = 0.9 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * rng.uniform(2.0, 6.0) ** 2)) + 0.2 * val
    elif kind == 2:                                           # a few values: exact ties
        val = np.round(val * int(rng.integers(3, 9))) / 8.0
    val = val.astype(np.float32)
    uv = af.line_pivots(lu, lv)
    case = (None, None, None, None, np.array([0, len(uv)]), uv, OCW)
    return val, af.speculative_climbs(case, 0, val), (abs(lu) + 2, abs(lv) + 2)


def test_rule_equals_the_sequential_loop_on_random_surfaces():
    rng = np.random.default_rng(20261020)
    seen = collections.Counter()
    for i in range(N_SURFACES):
        val, climbs, start = random_point(rng, i)
        seen[(i // 8) % 3, rc.check_point(val.tolist(), climbs, start)] += 1
    for kind, name in enumerate(("bump", "noise", "quantised")):
        print(name, {o: seen[kind, o] for o in rc.OUTCOMES})
        assert seen[kind, "short"] >= 100 and seen[kind, "short_u"] >= 100 and seen[kind, "fell_back"] >= 100, (name, seen)


@functools.lru_cache(maxsize=None)
def fixture_classes():
    """points per class over all GPU fixtures; every point is checked against the sequential loop on the way"""
    total = collections.Counter()
    for ocw in rc.OCWS:
        for name, _ in rc.FIXTURES:
            n = collections.Counter()
            for val, climbs, start, cls, _ in rc.fixture_points(name, ocw):
                rc.check_point(val, climbs, start)
                n.update(cls)
            print("ocw", ocw, name, {c: n[c] for c in rc.CLASSES if n[c]})
            total.update(n)
    print("all fixtures", {c: total[c] for c in rc.CLASSES})
    return total


def test_gpu_fixture_points_obey_the_rule():
    assert sum(fixture_classes().values()) >= 400


@pytest.mark.parametrize("cls", rc.CLASSES)
def test_gpu_fixtures_hold_every_class(cls):
    """each class holds at least five points of the GPU fixtures.  "Cut under U but not in reality" needs a pivot in front of the
    winner that is itself cut in reality AND whose unperformed scans cover a whole scan of the winner: with pivots along a line, 1 of
    6,000 of the random surfaces above holds one and none of 4,552 points searched on dense grids over the independent-noise and
    quantised pairs, so the "cuts" fixture carries eight points with hand-made pivot lists for it (rc.CUT_U_POINTS)."""
    total = fixture_classes()
    print(cls, total[cls])
    assert total[cls] >= 5, (cls, dict(total))
