"""Test infrastructure of NCC stacking (mimc3_stack_*): the definition of include/mimc3_hip.h restated in numpy -- sequential f64 adds in
layer order, the counts, the mean surface -- with the tail of tests/full_any_common.py behind it, and the noisy series the CPU test and
tools/stack_demo.py share."""
import numpy as np

from full_any_common import tail_from_surface
from full_fb_common import FB_OFFSET, FB_TRUE, fb_points

SHAPES = ((7, 4), (16, 15), (40, 6))    # (ocw, R)


class NumpyStack:
    """The stack by its definition: add() layers in order, finish() any number of times."""

    def __init__(self, n, radius, shift=None):
        self.n, self.radius, self.cells = int(n), int(radius), (2 * int(radius) + 1) ** 2
        self.shift = np.zeros((self.n, 2), np.int32) if shift is None else np.ascontiguousarray(shift, np.int32).copy()
        self.sum = np.zeros((self.n, self.cells), np.float64)
        self.cnt = np.zeros((self.n, self.cells), np.uint16)
        self.lay = np.zeros(self.n, np.uint16)
        self.layers = 0

    def add(self, surf, refused=None):
        """One layer: surf float32[n][cells]; refused bool[n] or None."""
        surf = np.asarray(surf, np.float32)
        assert surf.shape == (self.n, self.cells)
        fin = np.isfinite(surf)
        self.sum[fin] += surf[fin].astype(np.float64)            # one f64 addition per cell and layer, in layer order
        self.cnt[fin] += 1
        taken = np.ones(self.n, bool) if refused is None else ~np.asarray(refused, bool)
        self.lay[taken] += 1
        self.layers += 1
        return self

    def mean(self, min_count=1):
        ok = self.cnt >= max(int(min_count), 1)
        m = np.full((self.n, self.cells), np.nan, np.float32)
        m[ok] = (self.sum[ok] / self.cnt[ok].astype(np.float64)).astype(np.float32)     # f64 division, rounded once
        return m

    def finish(self, npeaks=0, min_count=1):
        """-> (record float32[n][8], candidates float32[npeaks][n][3] or None, lay uint16[n], mean float32[n][cells])"""
        m = self.mean(min_count)
        rec, cand = tail_from_surface(m, self.shift, self.radius, npeaks, refused=self.lay == 0, device_snr_order=True)
        return rec, cand, self.lay.copy(), m


def refused_of(record):
    """The refused flag of a layer that came from the search: status -3 in the record."""
    return np.asarray(record)[:, 2] == -3


def misplaced(record, truth, tol=0.5):
    """bool[n]: no fit, or the fitted displacement more than tol px (either axis) from truth (du, dv)."""
    du, dv = record[:, 0], record[:, 1]
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(du) & np.isfinite(dv) & (np.abs(du - truth[0]) <= tol) & (np.abs(dv - truth[1]) <= tol))


# ---- the noisy series: one motion, independent texture and noise per pair ----
SERIES_OCW, SERIES_R, SERIES_PAIRS, SERIES_NOISE_DN = 7, 4, 6, 100
SERIES_TRUTH = (FB_TRUE[0] - FB_OFFSET[0], FB_TRUE[1] - FB_OFFSET[1])      # the record's (du, dv) is relative to uv0 + offset


def series_pairs(pairs=SERIES_PAIRS, noise_dn=SERIES_NOISE_DN, H=160, W=160):
    """`pairs` 8-bit pairs (synth.make_pair) that all moved by FB_TRUE, each with its own texture and its own uniform noise of
    +-noise_dn DN on image 1"""
    from mimc3_amd import synth
    return [synth.make_pair(H, W, FB_TRUE, 100 + 17 * k, noise_dn=noise_dn) for k in range(pairs)]


def series_points(ocw=SERIES_OCW, radius=SERIES_R):
    """fb_points' 60 points and shift: the true peak lies on an interior cell everywhere but at point 56, where it lies on the border"""
    return fb_points(ocw=ocw, radius=radius)
