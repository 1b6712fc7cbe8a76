"""Test infrastructure: image pairs whose null pixels are not +0.0, and points placed at the 80 % invalid-pixel limit.

The reference's rule (MIMC_module.c) has three parts:
  * :723      a pixel enters the NCC sums only if x >= MIN_DN (1e-10, a double: f32 pixels are promoted);
  * :622/:631 a pixel is invalid if x < MIN_DN -- NaN is NOT counted there (every comparison with NaN is false), yet :723 still
              excludes it; the point is -3 if (float)count / (float)npx > 0.8f for the chip or for the whole Dy2 x Dx2 search area,
              whose never-written last row and column (T4) are zeros, i.e. Dx2 + Dy2 - 1 more invalid pixels;
  * :2545     GMA_float_conv2 treats a pixel as null iff (int32_t)(p + 0.5) == 0, i.e. -1.5 < p < 0.5.
"""
import dataclasses

import numpy as np

from mimc3_amd import synth


def _thr():
    """The smallest f32 whose f64 value is >= 1e-10: "x >= MIN_DN" is exactly "x >= THR" in f32."""
    t = np.float32(1e-10)
    if float(t) < 1e-10:
        t = np.nextafter(t, np.float32(1))
    return np.float32(t)


THR = _thr()
BELOW_THR = np.nextafter(THR, np.float32(0))          # the largest f32 whose f64 value is below 1e-10
assert float(BELOW_THR) < 1e-10 <= float(THR)

# null encodings: name -> f32 bits (NaN payloads and the sign of zero are kept exactly)
ENCODINGS = {
    "zero": np.float32(0.0),
    "negzero": np.float32(-0.0),
    "minus1": np.float32(-1.0),
    "m9999": np.float32(-9999.0),
    "neginf": np.float32(-np.inf),
    "nan": np.uint32(0x7FC00000).view(np.float32),
    "negnan": np.uint32(0xFFC00000).view(np.float32),
    "1e-11": np.float32(1e-11),
    "below_thr": BELOW_THR,
}
U8_ENCODINGS = ("zero", "negzero")                    # pass "v >= 0 and integral": the pair stays 8-bit
NOT_COUNTED = ("nan", "negnan")                       # excluded from the sums (:723) but not counted invalid (:622/:631)

# a few points per chip size; corridors of a handful of pivots (every kernel path takes them)
GEOM = {
    7: dict(h=160, w=176, dimx=9, dimy=8, speed=1200.0),
    15: dict(h=220, w=230, dimx=6, dimy=6, speed=1500.0),
    16: dict(h=240, w=250, dimx=6, dimy=6, speed=1500.0),
    30: dict(h=300, w=320, dimx=5, dimy=4, speed=700.0),
    32: dict(h=320, w=330, dimx=5, dimy=4, speed=700.0),
    40: dict(h=360, w=340, dimx=4, dimy=4, speed=900.0),
}


def fill(img, mask, value):
    out = np.array(img, np.float32, copy=True)
    out[mask] = value
    return out


def base_case(ocw, null_frac=0.08):
    """Integral 8-bit DN with +0.0 null blobs in both images (synth), offset (1, -1)."""
    return synth.make_small(seed=8000 + ocw, shift=(2, -3), angle_deg=35.0, ocw=ocw, noise_dn=2, null_frac=null_frac,
                            offset=(1, -1), **GEOM[ocw])


def encoded_case(ocw, enc):
    """base_case with every null pixel re-encoded as ENCODINGS[enc]."""
    c = base_case(ocw)
    v = ENCODINGS[enc]
    return dataclasses.replace(c, i0=fill(c.i0, c.i0 == 0, v), i1=fill(c.i1, c.i1 == 0, v))


def threshold_case(ocw, frac=0.05):
    """base_case plus valid pixels equal to THR (the smallest valid f32) at ~frac of the non-null pixels of each image."""
    c = base_case(ocw)
    rng = np.random.default_rng(900 + ocw)
    i0 = fill(c.i0, (c.i0 > 0) & (rng.random(c.i0.shape) < frac), THR)
    i1 = fill(c.i1, (c.i1 > 0) & (rng.random(c.i1.shape) < frac), THR)
    return dataclasses.replace(c, i0=i0, i1=i1)


def inf_case(ocw, count=12):
    """base_case plus +inf at `count` pixels of each image, inside the area the points' chips and windows cover."""
    c = base_case(ocw)
    rng = np.random.default_rng(700 + ocw)
    u = c.xyuvav[:, 2].astype(int); v = c.xyuvav[:, 3].astype(int)
    imgs = []
    for img in (c.i0, c.i1):
        img = img.copy()
        pick = rng.choice(len(u), size=count)
        img[v[pick] + rng.integers(-ocw, ocw + 1, count), u[pick] + rng.integers(-ocw, ocw + 1, count)] = np.inf
        imgs.append(img)
    return dataclasses.replace(c, i0=imgs[0], i1=imgs[1])


def last_pixel_case(enc):
    """A null-free 8-bit pair but for ONE null, the last pixel of image 1 (the grid-stride tails of the pair's classifiers)."""
    c = synth.make_small(seed=8100, shift=(3, -2), angle_deg=20.0, ocw=7)
    i1 = c.i1.copy()
    i1[-1, -1] = ENCODINGS[enc]
    return dataclasses.replace(c, i1=i1)


# ---- the 80 % limit ---------------------------------------------------------------------------------------------------------------
def first_invalid_count(npx):
    """The first count k with (float)k / (float)npx > 0.8f (MIMC_module.c:635, f32 throughout)."""
    r = np.float32(0.8)
    k = int(0.8 * npx) - 2
    while not (np.float32(k) / np.float32(npx) > r):
        k += 1
    return k


@dataclasses.dataclass
class LimitCase:
    chip_img: np.ndarray      # [H][W] f32: the image the chips come from
    win_img: np.ndarray       # [H][W] f32: the image the search areas come from
    xyuvav: np.ndarray
    offset: np.ndarray
    piv_off: np.ndarray       # None for the exhaustive search
    piv_uv: np.ndarray
    ocw: int
    labels: list              # per point: (side, count, k); count None = every pixel of that side null
    radius: int = 0

    def expect_invalid(self, counted=True):
        """The -3 mask the rule gives: flips exactly at k; nothing flips when the nulls are not counted (NaN)."""
        return np.array([counted and (n is None or n >= k) for _, n, k in self.labels])


def _layout(span, n, cols=4):
    """Point centres on a grid with `span` px between them: no two points' chips or search areas share a pixel."""
    rows = (n + cols - 1) // cols
    H, W = (rows + 2) * span, (cols + 2) * span
    cu = [span + span // 2 + span * (i % cols) for i in range(n)]
    cv = [span + span // 2 + span * (i // cols) for i in range(n)]
    return H, W, np.array(cu), np.array(cv)


def limit_case(ocw, enc, pivots=None, radius=0, seed=0):
    """Points with exactly k - 1, k and k + 1 invalid pixels in the chip, and in the search area, plus one point whose chip and one
    whose search area is null throughout.  Nulls are ENCODINGS[enc]; every other pixel is integral 8-bit DN.

    DLC matcher (radius 0): every point has the zero velocity, i.e. the pivots (0, 0) .. (10, 0) (AW_CRE + 1 of them), so
    Dx2 = 2 (ocw + 12) + 1, Dy2 = 2 (ocw + 2) + 1; the count of the search area includes its never-written last row and column
    (T4, Dx2 + Dy2 - 1 zeros), and the written nulls are placed both away from and on the last written row and column.
    `pivots(xyuvav, ocw, H, W) -> (piv_off, piv_uv)` gives the pivots (the test's oracle).
    Exhaustive search (radius R): the search box is the (2 (R + ocw) + 1)^2 square around uv0 + offset, all written (no T4 term)."""
    cw = 2 * ocw + 1
    full = radius > 0
    if full:
        Dx2 = Dy2 = 2 * (radius + ocw) + 1
        t4 = 0
    else:
        Dx2, Dy2 = 2 * (ocw + 12) + 1, 2 * (ocw + 2) + 1
        t4 = Dx2 + Dy2 - 1
    kc, kw = first_invalid_count(cw * cw), first_invalid_count(Dx2 * Dy2)
    labels = [("chip", kc + d, kc) for d in (-1, 0, 1)]
    labels += [("win_inner" if not full else "win", kw + d, kw) for d in (-1, 0, 1)]
    if not full:
        labels += [("win_edge", kw + d, kw) for d in (-1, 0, 1)]
    labels += [("chip", None, kc), ("win", None, kw)]
    n = len(labels)
    span = max(Dx2, Dy2, cw) + 6
    H, W, cu, cv = _layout(span, n)
    rng = np.random.default_rng(seed * 1000 + ocw)
    base = synth.texture(H + 4, W + 4, 4200 + ocw)
    chip_img = np.ascontiguousarray(base[2:H + 2, 2:W + 2])
    win_img = base[1:H + 1, 4:W + 4] + rng.integers(-2, 3, (H, W)).astype(np.float32)   # the peak near (du, dv) = (-2, 1)
    win_img = np.ascontiguousarray(np.clip(win_img, 1, 255))
    null = ENCODINGS[enc]
    for (side, cnt, _), u, v in zip(labels, cu, cv):
        if side == "chip":
            sub = chip_img[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1]
            idx = np.arange(cw * cw) if cnt is None else rng.choice(cw * cw, cnt, replace=False)
            sub[np.unravel_index(idx, sub.shape)] = null          # (sub is a view: reshape would copy)
            continue
        # the search area's top-left pixel sits at uv0 - (Dx2 / 2, Dy2 / 2); for the DLC matcher its last row and column are not written
        wx, wy = (Dx2, Dy2) if full else (Dx2 - 1, Dy2 - 1)
        sub = win_img[v - Dy2 // 2:v - Dy2 // 2 + wy, u - Dx2 // 2:u - Dx2 // 2 + wx]
        if cnt is None:
            sub[:] = null
            continue
        need = cnt - t4
        if side == "win_edge":                  # the last written row and column first, the rest anywhere
            sub[-1, :] = null; sub[:, -1] = null
            inner = sub[:-1, :-1].reshape(-1).copy()
            inner[rng.choice(inner.size, need - (wx + wy - 1), replace=False)] = null
            sub[:-1, :-1] = inner.reshape(wy - 1, wx - 1)
        elif side == "win_inner":               # none on the last written row or column
            inner = sub[:-1, :-1].reshape(-1).copy()
            inner[rng.choice(inner.size, need, replace=False)] = null
            sub[:-1, :-1] = inner.reshape(wy - 1, wx - 1)
        else:
            sub[np.unravel_index(rng.choice(sub.size, need, replace=False), sub.shape)] = null
    xy = np.zeros((n, 6))
    xy[:, 2] = cu; xy[:, 3] = cv
    xy[:, 0] = cu * synth.MPP; xy[:, 1] = -cv * synth.MPP
    offset = np.zeros(2, np.int32)
    piv_off = piv_uv = None
    if not full:
        piv_off, piv_uv = pivots(xy, ocw, H, W)
        last = piv_uv[piv_off[1:] - 1]
        assert (np.abs(last[:, 0]) == 10).all() and (last[:, 1] == 0).all(), "the zero velocity no longer gives pivots (0..10, 0)"
    return LimitCase(chip_img, win_img, xy, offset, piv_off, piv_uv, ocw, labels, radius)


def count_invalid(case):
    """Recount each point's invalid pixels (x < 1e-10 in f64, NaN not counted) from the images as the reference reads them."""
    out = []
    cw = 2 * case.ocw + 1
    full = case.radius > 0
    Dx2 = Dy2 = 2 * (case.radius + case.ocw) + 1
    if not full:
        Dx2, Dy2 = 2 * (case.ocw + 12) + 1, 2 * (case.ocw + 2) + 1
    for (side, _, _), (u, v) in zip(case.labels, case.xyuvav[:, 2:4].astype(int)):
        if side == "chip":
            a = case.chip_img[v - case.ocw:v + case.ocw + 1, u - case.ocw:u + case.ocw + 1].astype(np.float64)
        else:
            a = case.win_img[v - Dy2 // 2:v - Dy2 // 2 + Dy2, u - Dx2 // 2:u - Dx2 // 2 + Dx2].astype(np.float64)
            if not full:
                a = a.copy(); a[-1, :] = 0; a[:, -1] = 0          # T4: never written
        out.append(int((a < 1e-10).sum()))
    return out


# ---- the pre-filter and the control-point stage ----------------------------------------------------------------------------------
# GMA_float_conv2's null test (int32_t)(p + 0.5) == 0 on both sides of both ends, NaN, a valid negative, and a value whose
# (int32_t) conversion is out of range (x86-64: INT_MIN, i.e. "not null")
CONV2_EDGES = (np.float32(-1.5), np.nextafter(np.float32(-1.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(0)),
               np.float32(0.5), ENCODINGS["nan"], np.float32(-9999.0), np.float32(3e9))
HUGE = np.float32(3e9)


def sprinkle(img, values, frac, rng):
    """img with each of `values` at ~frac of the pixels (disjoint picks)."""
    out = np.array(img, np.float32, copy=True)
    pick = rng.permutation(out.size)
    per = max(1, int(frac * out.size))
    for i, v in enumerate(values):
        out.reshape(-1)[pick[i * per:(i + 1) * per]] = v
    return out


def conv2_case(huge=True):
    """An 8-bit pair (ocw 7, +0.0 null blobs) with every CONV2_EDGES value at ~0.5 % of the pixels of each image (3e9 left out
    when not `huge`: its square is far beyond 2^53, so the matcher's f64 sums of the filtered pair would depend on their order)."""
    c = synth.make_small(seed=8200, shift=(2, 1), angle_deg=-30.0, ocw=7, null_frac=0.04)
    rng = np.random.default_rng(8201)
    vals = [v for v in CONV2_EDGES if huge or v != HUGE]
    return dataclasses.replace(c, i0=sprinkle(c.i0, vals, 0.005, rng), i1=sprinkle(c.i1, vals, 0.005, rng))


CP_KERNELS = [np.array([[-1, 0, 1]], np.float32), np.array([[-1], [0], [1]], np.float32),
              np.array([[-1 / 8] * 3, [-1 / 8, 1, -1 / 8], [-1 / 8] * 3], np.float32)]


def cp_case(enc, seed=2, h=620, w=700, dimx=24, dimy=20):
    """The control-point stage's input (as tests/test_cp_offset_parity.py: 5 % null blobs, noise, 70 % slow points) with its nulls
    encoded as ENCODINGS[enc]."""
    i0, i1 = synth.make_pair(h, w, (-3, 4), seed=seed, null_frac=0.05, noise_dn=2)
    xy = synth.make_grid(dimx, dimy, 60, 60, (w - 120) // dimx, (h - 120) // dimy, 1806.0, angle_deg=30.0)
    rng = np.random.default_rng(seed)
    s = rng.random(dimx * dimy) < 0.7
    xy[s, 4] = rng.uniform(-5, 5, s.sum()); xy[s, 5] = rng.uniform(-5, 5, s.sum())
    v = ENCODINGS[enc]
    return fill(i0, i0 == 0, v), fill(i1, i1 == 0, v), xy
