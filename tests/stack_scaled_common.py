"""Test infrastructure of the scaled and weighted layers of NCC stacking (mimc3_stack_add_scaled, mimc3_stack_add_surfaces_scaled): the
definition of include/mimc3_hip.h restated in numpy on top of NumpyStack (tests/stack_common.py) -- the layer shift, the bilinear taps in
f64 in the header's order of operations, the weights' sums, the weighted mean -- and the noisy series over six time baselines that the
CPU test, the GPU test and tools/stack_scaled_time.py share."""
import numpy as np

from full_fb_common import FB_OFFSET, fb_points
from stack_common import NumpyStack

SCALE_MIN, SCALE_MAX = 2.0 ** -6, 2.0 ** 6


def layer_radius(radius, scale):
    """mimc3_stack_layer_radius"""
    return int(radius) if scale == 1 else int(np.floor(np.float64(scale) * np.float64(radius) + 0.5)) + 1


def layer_shift(shift, scale):
    """mimc3_stack_layer_shift: one f64 product, rint (half to even)"""
    return np.rint(np.float64(scale) * np.asarray(shift, np.int32).astype(np.float64)).astype(np.int32)


def axis_taps(shift, lshift, radius, layer_r, scale):
    """One axis of every point -> (a float64[n][S], j int64[n][S]): the fraction and the first tap of every stack cell along it"""
    d = np.arange(-radius, radius + 1, dtype=np.int64)
    p = np.float64(scale) * (shift.astype(np.int64)[:, None] + d[None, :]).astype(np.float64) - lshift.astype(np.float64)[:, None]
    f = np.floor(p)
    return p - f, f.astype(np.int64) + layer_r


def resample(surf, layer_r, shift, radius, scale):
    """A layer's surfaces float32[n][Sl^2] on the stack's cells -> (value float64[n][S^2], read bool[n][S^2], taps int[n][S^2]): value where
    every tap that is read lies inside the layer (read), NaN elsewhere; taps is how many taps the cell reads (1, 2 or 4)"""
    n, S, Sl = surf.shape[0], 2 * radius + 1, 2 * layer_r + 1
    L = np.asarray(surf, np.float32).reshape(n, Sl, Sl).astype(np.float64)
    shift = np.asarray(shift, np.int32)
    lsh = layer_shift(shift, scale)
    au, ju = axis_taps(shift[:, 0], lsh[:, 0], radius, layer_r, scale)
    av, jv = axis_taps(shift[:, 1], lsh[:, 1], radius, layer_r, scale)
    au, ju, av, jv = au[:, :, None], ju[:, :, None], av[:, None, :], jv[:, None, :]        # [n][S][1] and [n][1][S]
    two_u, two_v = au != 0, av != 0
    read = (ju >= 0) & (jv >= 0) & (ju + two_u < Sl) & (jv + two_v < Sl)
    pt = np.arange(n)[:, None, None]
    j0, j1, i0, i1 = np.clip(ju, 0, Sl - 1), np.clip(ju + 1, 0, Sl - 1), np.clip(jv, 0, Sl - 1), np.clip(jv + 1, 0, Sl - 1)
    with np.errstate(invalid="ignore"):

        def row(j):
            return np.where(two_v, (1 - av) * L[pt, j, i0] + av * L[pt, j, i1], L[pt, j, i0])

        value = np.where(two_u, (1 - au) * row(j0) + au * row(j1), row(j0))
    value = np.where(read, value, np.nan)
    taps = (1 + two_u) * (1 + two_v) * np.ones((n, S, S), np.int64)
    return value.reshape(n, S * S), np.broadcast_to(read, (n, S, S)).reshape(n, S * S), taps.reshape(n, S * S)


class NumpyScaledStack(NumpyStack):
    """NumpyStack with the scaled and weighted layers: add() and add_scaled() in any order, finish() any number of times."""

    def __init__(self, n, radius, shift=None):
        super().__init__(n, radius, shift)
        self.wsum = None                                         # float64[n][cells] once the stack is weighted

    @property
    def weighted(self):
        return self.wsum is not None

    def add(self, surf, refused=None):
        if self.weighted:
            self.wsum[np.isfinite(np.asarray(surf, np.float32))] += 1.0
        return super().add(surf, refused)

    def add_scaled(self, surf, radius, scale, weight=1.0, refused=None):
        """One scaled layer: surf float32[n][(2 radius + 1)^2], searched around layer_shift(self.shift, scale)"""
        scale, weight, radius = np.float64(scale), np.float64(weight), int(radius)
        assert SCALE_MIN <= scale <= SCALE_MAX and np.isfinite(weight) and weight > 0 and 1 <= radius <= 47
        surf = np.asarray(surf, np.float32)
        assert surf.shape == (self.n, (2 * radius + 1) ** 2)
        assert (np.abs(scale * self.shift.astype(np.float64)) < 2.0 ** 30).all()
        if weight != 1.0 and not self.weighted:
            self.wsum = self.cnt.astype(np.float64)
        value, _, _ = resample(surf, radius, self.shift, self.radius, scale)
        fin = np.isfinite(value)
        self.sum[fin] += weight * value[fin]                     # one product, one addition
        self.cnt[fin] += 1
        if self.weighted:
            self.wsum[fin] += weight
        taken = np.ones(self.n, bool) if refused is None else ~np.asarray(refused, bool)
        self.lay[taken] += 1
        self.layers += 1
        return self

    def mean(self, min_count=1):
        if not self.weighted:
            return super().mean(min_count)
        ok = self.cnt >= max(int(min_count), 1)
        m = np.full((self.n, self.cells), np.nan, np.float32)
        m[ok] = (self.sum[ok] / self.wsum[ok]).astype(np.float32)                        # f64 division, rounded once
        return m


# ---- the noisy series over six time baselines: one velocity, independent texture and noise per pair ----
SCALED_OCW, SCALED_R, SCALED_NOISE_DN = 7, 4, 100
SCALED_SCALES = (1.0, 2.0, 0.5, 3.0, 1.5, 2.0)
SCALED_MOTION = (2.0, -1.0)              # px in the stack's interval, relative to FB_OFFSET: layer k moved scale_k times this
SCALED_COUNTS = ([28, 22, 25, 27, 24, 21], 1, 58)       # misplaced of 60: per layer (own truth), the scaled stack, the unscaled stack


def scaled_series_pairs(noise_dn=SCALED_NOISE_DN, H=160, W=160):
    """[(scale, i0, i1)]: 8-bit pairs (synth.make_pair, seed 100 + 17 k, +-noise_dn DN of uniform noise on image 1) that moved by
    FB_OFFSET + scale * SCALED_MOTION; the integer part is floor(total + 1e-9), the rest is the pair's subpixel motion"""
    from mimc3_amd import synth
    out = []
    for k, s in enumerate(SCALED_SCALES):
        tot = np.asarray(FB_OFFSET, np.float64) + s * np.asarray(SCALED_MOTION)
        ish = np.floor(tot + 1e-9).astype(int)
        i0, i1 = synth.make_pair(H, W, ish, 100 + 17 * k, subpixel=tuple(tot - ish), noise_dn=noise_dn)
        out.append((s, i0, i1))
    return out


def scaled_series_points():
    """fb_points' 60 points and shift at ocw 7, R 4 (point 56: the true peak on the border of its box)"""
    return fb_points(ocw=SCALED_OCW, radius=SCALED_R)


def layer_truth(scale):
    return (scale * SCALED_MOTION[0], scale * SCALED_MOTION[1])
