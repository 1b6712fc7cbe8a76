"""Test infrastructure: the coarse-to-fine exhaustive search on every pair class (mimc3_match_ncc_pyramid_dn, include/mimc3_hip.h) restated
on the CPU on float pixels -- the 2 x 2 reduction on the integers w = pixel * 2^s in numpy int64, every level's search through
full_dn_common.full_dn's surface (arg-max = the lowest k among the largest finite cells, -1 where there is none), the chip and
border rules of pyramid_oracle._inside, and level 0 through full_dn with its candidates."""
import numpy as np

from full_dn_common import full_dn
from pyramid_oracle import _inside


def image_shift(img):
    """The shift s of an image: 0 when every pixel is an integer, 3 when every pixel is a multiple of 1/8 (the classes' two scales)."""
    a = np.asarray(img, np.float32)
    if (a == np.rint(a)).all():
        return 0
    assert (a * 8 == np.rint(a * 8)).all(), "neither integers nor multiples of 1/8"
    return 3


def reduce2_dn(img, s):
    """One level: pixel = ((sum w + n // 2) // n) / 2^s over the n non-zero w = pixel * 2^s of the 2 x 2 block, 0 when n = 0; an odd last
    row or column is dropped."""
    w = np.asarray(img, np.float64) * (1 << s)
    a = np.rint(w).astype(np.int64)
    assert (a == w).all() and a.min() >= 0
    H, W = a.shape[0] >> 1, a.shape[1] >> 1
    b = a[:2 * H, :2 * W].reshape(H, 2, W, 2)
    n = (b != 0).sum(axis=(1, 3))
    t = b.sum(axis=(1, 3))
    m = np.where(n > 0, (t + n // 2) // np.maximum(n, 1), 0)
    return np.ascontiguousarray((m / float(1 << s)).astype(np.float32))          # (m < 2^20: exact)


def pyramid_dn(img, levels):
    """[level 0 (the image), level 1, ...]; every level inherits level 0's shift."""
    s = image_shift(img)
    out = [np.ascontiguousarray(img, np.float32)]
    for _ in range(1, levels):
        out.append(reduce2_dn(out[-1], s))
    return out


def surface_peaks(surf):
    """arg-max per point of float32[N][S * S] surfaces in k order: the lowest k among the largest finite cells, -1 without a finite cell."""
    v = np.where(np.isfinite(surf), surf, -np.inf)
    pk = v.argmax(axis=1).astype(np.int64)                     # (numpy's argmax returns the first of equals: the lowest k)
    pk[~np.isfinite(surf).any(axis=1)] = -1
    return pk


def level_peaks_dn(i0l, i1l, pos, d, ocw, R, swap=False):
    """The arg-max k of the exhaustive search on one level at pos with offset 0 and shift d (-1 where there is none)."""
    H, W = i0l.shape
    ok = _inside(pos, d, ocw, R, H, W)
    peak = np.full(pos.shape[0], -1, np.int64)
    if ok.any():
        xy = np.zeros((int(ok.sum()), 6))
        xy[:, 2:4] = pos[ok]
        surf = full_dn(i0l, i1l, xy, (0, 0), ocw, R, 0, shift=d[ok].astype(np.int32), swap=swap, with_surface=True)[2]
        peak[ok] = surface_peaks(surf)
    return peak


def pyramid_search_dn(i0, i1, xyuvav, offset, ocw, radius, levels, npeaks=0, shift=None, swap=False, with_peaks=False):
    """-> (float32[N][8] record, float32[npeaks][N][3] candidates or None, int32[N][2] shift_out), the definition step by step; with_peaks
    appends the list of the coarser levels' arg-max cells, coarsest first."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    off = np.asarray(offset, np.int64).reshape(1, 2)
    D = off + (np.zeros((n, 2), np.int64) if shift is None else np.asarray(shift, np.int64))
    uv0 = xy[:, 2:4].astype(np.int64)                          # (int) truncation
    L = int(levels)
    d = D if L == 1 else (D + (1 << (L - 2))) >> (L - 1)       # floor((D + 2^(L-2)) / 2^(L-1))
    p0, p1 = pyramid_dn(i0, L), pyramid_dn(i1, L)
    S = 2 * radius + 1
    peaks = []
    for lv in range(L - 1, 0, -1):
        pk = level_peaks_dn(p0[lv], p1[lv], uv0 >> lv, d, ocw, radius, swap)
        peaks.append(pk)
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - radius, pk % S - radius], axis=1), 0)
        d = 2 * (d + s)
    shift_out = (d - off).astype(np.int32)
    rec, cand = full_dn(i0, i1, xy, offset, ocw, radius, npeaks, shift=shift_out, swap=swap)
    H, W = np.asarray(i0).shape
    out = ~_inside(uv0, d, ocw, radius, H, W)
    rec[out] = np.nan
    if cand is not None:
        cand[:, out] = np.nan
    res = (rec, cand, shift_out)
    return res + (peaks,) if with_peaks else res


def dn12_low(img, seed):
    """An 8-bit image (0 = null) -> 12-bit DN with low-order entropy: 16 * pixel + 4 random low bits; nulls stay 0, the maximum is <= 4095."""
    img = np.asarray(img, np.float32)
    low = np.random.default_rng(seed).integers(0, 16, img.shape).astype(np.float32)
    out = np.where(img == 0, np.float32(0), img * np.float32(16) + low).astype(np.float32)
    assert out.max() <= 4095 and out.max() > 255 and ((out == 0) == (img == 0)).all()
    return np.ascontiguousarray(out)


def case(ocw, null_frac, seed, levels=3):
    """The parity fixture of tests/test_full_search_pyramid.py: odd image sizes (the reductions drop a row and a column), a coarsest level
    that holds a chip, a motion the prior misses by a few px; 30 points."""
    from mimc3_amd import synth
    h = (2 * ocw + 1) * (1 << (levels - 1)) + 45
    return synth.make_small(seed=seed, shift=(9, -7), angle_deg=40.0, ocw=ocw, speed=700.0, h=h, w=h + 14, dimx=6, dimy=5,
                            noise_dn=2, null_frac=null_frac, offset=(1, -1), sigma=3.0)


def as_class(cls, c, seed=0):
    """The 8-bit pair of a case as 12-bit DN with low-order entropy ("u16") or as full-entropy 16-bit DN ("f32") -> (i0, i1)"""
    from full_dn_common import to_dn16
    if cls == "u16":
        return dn12_low(c.i0, 3000 + seed), dn12_low(c.i1, 4000 + seed)
    assert cls == "f32"
    return to_dn16(c.i0, 1000 + seed), to_dn16(c.i1, 2000 + seed)
