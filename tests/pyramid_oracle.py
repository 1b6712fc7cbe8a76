"""Test infrastructure: the coarse-to-fine exhaustive search (mimc3_match_ncc_pyramid, include/mimc3_hip.h) restated on the CPU -- the
2 x 2 reduction in numpy with exact integers, every level's search through full_search_common.full_search (its arg-max k, -1 without
one), and the two rules full_search does not model applied here: a point whose chip leaves a level's image, or whose search box leaves
that level's 256-px zero border, has no arg-max there (and gets the all-NaN record on level 0)."""
import numpy as np

from full_search_common import full_search
from mimc3_amd import synth

PAD = 256          # the planes' zero border (kU8Pad)


def reduce2(img):
    """One pyramid level: pixel (x, y) = (s + n // 2) // n over the n non-zero pixels (sum s) of the 2 x 2 block at (2x, 2y), 0 if n = 0;
    an odd last row or column is dropped."""
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape[0] >> 1, a.shape[1] >> 1
    b = a[:2 * H, :2 * W].reshape(H, 2, W, 2)
    n = (b != 0).sum(axis=(1, 3))
    s = b.sum(axis=(1, 3))
    return np.where(n > 0, (s + n // 2) // np.maximum(n, 1), 0).astype(np.float32)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, np.float32)]
    for _ in range(1, levels):
        out.append(reduce2(out[-1]))
    return out


def _inside(pos, d, ocw, R, H, W):
    """chip inside the image and search box inside the zero border, per point (pos, d int64 [N][2])"""
    chip = (pos[:, 0] - ocw >= 0) & (pos[:, 0] + ocw < W) & (pos[:, 1] - ocw >= 0) & (pos[:, 1] + ocw < H)
    c, h = pos + d, R + ocw
    box = (c[:, 0] - h >= -PAD) & (c[:, 0] + h < W + PAD) & (c[:, 1] - h >= -PAD) & (c[:, 1] + h < H + PAD)
    return chip & box


def level_peaks(i0l, i1l, pos, d, ocw, R, swap=False):
    """The arg-max k of the exhaustive search on one level at pos with offset 0 and shift d (-1 where there is none)."""
    H, W = i0l.shape
    ok = _inside(pos, d, ocw, R, H, W)
    peak = np.full(pos.shape[0], -1, np.int64)
    if ok.any():
        xy = np.zeros((int(ok.sum()), 6))
        xy[:, 2:4] = pos[ok]
        _, pk = full_search(i0l, i1l, xy, (0, 0), ocw, R, shift=d[ok].astype(np.int32), swap=swap, with_peak=True)
        peak[ok] = pk
    return peak


def pyramid_search(i0, i1, xyuvav, offset, ocw, radius, levels, shift=None, swap=False):
    """-> (float32[N][8] record, int32[N][2] shift_out), the definition of include/mimc3_hip.h step by step."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    off = np.asarray(offset, np.int64).reshape(1, 2)
    D = off + (np.zeros((n, 2), np.int64) if shift is None else np.asarray(shift, np.int64))
    uv0 = xy[:, 2:4].astype(np.int64)                          # (int) truncation
    L = int(levels)
    d = D if L == 1 else (D + (1 << (L - 2))) >> (L - 1)       # floor((D + 2^(L-2)) / 2^(L-1))
    p0, p1 = pyramid(i0, L), pyramid(i1, L)
    S = 2 * radius + 1
    for lv in range(L - 1, 0, -1):
        pk = level_peaks(p0[lv], p1[lv], uv0 >> lv, d, ocw, radius, swap)
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - radius, pk % S - radius], axis=1), 0)
        d = 2 * (d + s)
    shift_out = (d - off).astype(np.int32)
    rec = full_search(i0, i1, xy, offset, ocw, radius, shift=shift_out, swap=swap)
    H, W = np.asarray(i0).shape
    rec[~_inside(uv0, d, ocw, radius, H, W)] = np.nan
    return rec, shift_out


# the large-displacement case: a pair moved by (+70, -45) px, a smooth texture and 65-px chips, so that a level-2 search whose peak sits
# on the border of its +-15 box still points toward the motion
BIG = dict(h=801, w=811, ocw=32, sigma=4.0, motion=(70, -45))


def big_case():
    i0, i1 = synth.make_pair(BIG["h"], BIG["w"], BIG["motion"], 5, noise_dn=2, pad=128, sigma=BIG["sigma"])
    return i0, i1, synth.make_grid(8, 8, 150, 150, 70, 70, 0.0)
