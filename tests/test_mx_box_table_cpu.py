"""The table form of the clean form's window-side box sums (match_mx_kernel.hip, RecCfg; sat_cell_corners, sat_kernel.h), without a GPU:
the rule restated in numpy.  The packed table of a zero-bordered plane is built the way tests/u8_advance_common.null_table builds its
null table, with the three fields (b | b^2 << 21 | [b == 0] << 50, modulo 2^64); the query of every tile cell with its far corner
clamped to the never-written last column and row (T4) must equal the brute-force box sums of the window with that column and row
zeroed -- at all six chip sizes, on an ordinary plane, on a plane pressed against 255 (the field maxima at ocw 40) and for windows that
reach into the zero border.  Cells beyond the last reachable column or row are never read: their corners must stay inside the search
area."""
import numpy as np
import pytest

import u8_advance_common as ac

OCWS = (7, 15, 16, 30, 32, 40)
BORDER = 100
SQ, NUL = 21, 50           # kSatSqShift8, kSatNullShift8


def packed_table(img):
    H, W = img.shape
    f = np.zeros((H + 2 * BORDER + 1, W + 2 * BORDER + 1), np.uint64)
    b = img.astype(np.uint64)
    f[1:, 1:] = np.uint64(1) << np.uint64(NUL)                                   # the border is null
    f[BORDER + 1:BORDER + H + 1, BORDER + 1:BORDER + W + 1] = b | (b * b) << np.uint64(SQ) | (b == 0).astype(np.uint64) << np.uint64(NUL)
    with np.errstate(over="ignore"):
        return f.cumsum(0, dtype=np.uint64).cumsum(1, dtype=np.uint64)           # (modulo 2^64, as the device's)


def cell_corners(rx, ry, cw, xl, yl, zx, zy):
    """sat_cell_corners: (x, y, w, h) of the clamped query of tile cell (rx, ry), tile-relative"""
    x, y = min(rx, max(xl, 0)), min(ry, max(yl, 0))
    return x, y, max(min(cw, zx - x), 0), max(min(cw, zy - y), 0)


def query(S, px, py, w, h):
    """the box of plane pixels [px, px + w) x [py, py + h) (plane coordinates: the border included)"""
    with np.errstate(over="ignore"):
        q = int(S[py + h, px + w] - S[py, px + w] - S[py + h, px] + S[py, px])
    return q & ((1 << SQ) - 1), (q >> SQ) & ((1 << (NUL - SQ)) - 1), q >> NUL


def check_point(img, S, u0, v0, lu, lv, ocw):
    """every cell of the point's 32 x 32 tile; returns (cells compared, cells whose box meets the T4 column or row)"""
    cw = 2 * ocw + 1
    dx2, dy2 = abs(lu) + ocw + 2, abs(lv) + ocw + 2
    Dx2, Dy2, csx, csy = 2 * dx2 + 1, 2 * dy2 + 1, 2 * abs(lu) + 6, 2 * abs(lv) + 6
    fx, tx0, *_ = ac.axis_geometry(np.array([lu]), ocw)
    fy, ty0, *_ = ac.axis_geometry(np.array([lv]), ocw)
    tx0, ty0 = int(tx0[0]), int(ty0[0])
    wu0, wv0 = u0 - dx2 + BORDER, v0 - dy2 + BORDER                              # plane position of window pixel (0, 0)
    plane = np.zeros((img.shape[0] + 2 * BORDER, img.shape[1] + 2 * BORDER), np.int64)
    plane[BORDER:-BORDER, BORDER:-BORDER] = img
    win = plane[wv0:wv0 + Dy2, wu0:wu0 + Dx2].copy()
    assert win.shape == (Dy2, Dx2)
    win[-1, :] = 0
    win[:, -1] = 0
    zx, zy, xl, yl = Dx2 - 1 - tx0, Dy2 - 1 - ty0, csx - 2 - tx0, csy - 2 - ty0
    assert zx - cw + 1 == xl and zy - cw + 1 == yl
    n, t4 = 0, 0
    for ry in range(32):
        for rx in range(32):
            x, y, w, h = cell_corners(rx, ry, cw, xl, yl, zx, zy)
            # address safety, every cell: the corners lie inside the search area
            assert 0 <= x and x + w <= zx and 0 <= y and y + h <= zy and tx0 + zx == Dx2 - 1 and ty0 + zy == Dy2 - 1
            if tx0 + rx > csx - 2 or ty0 + ry > csy - 2:
                continue                                                          # beyond the last reachable cells: never read
            assert (x, y) == (rx, ry)
            s, ss, _ = query(S, wu0 + tx0 + x, wv0 + ty0 + y, w, h)
            b = win[ty0 + ry:ty0 + ry + cw, tx0 + rx:tx0 + rx + cw]
            assert b.shape == (cw, cw)
            assert (s, ss) == (int(b.sum()), int((b * b).sum())), (ocw, lu, lv, rx, ry)
            n += 1
            t4 += int(w < cw or h < cw)
    return n, t4


def planes(ocw):
    rng = np.random.default_rng(4100 + ocw)
    H, W = 2 * ocw + 150, 2 * ocw + 160
    ordinary = rng.integers(1, 256, (H, W)).astype(np.float32)
    ordinary[rng.random((H, W)) < 0.01] = 0                                      # nulls count as zeros in both sums
    high = np.full((H, W), 255, np.float32)
    high[rng.random((H, W)) < 0.02] = 254
    return ordinary, high


@pytest.mark.parametrize("ocw", OCWS)
def test_clamped_queries_equal_the_zeroed_window(ocw):
    ordinary, high = planes(ocw)
    H, W = ordinary.shape
    total = t4s = 0
    # (last pivots: a tile at origin 1 that holds the T4 cells; one whose grid is wider than the tile in x, so the centred tile ends in
    #  front of them; both signs)
    for img in (ordinary, high):
        S = packed_table(img)
        for lu, lv in ((5, -3), (-13, 9), (20, 2)):
            for u0, v0 in ((W // 2, H // 2), (ocw + 1, ocw + 2), (W - ocw - 2, H - ocw - 1)):      # inside; windows that reach into the border
                n, t4 = check_point(img, S, u0, v0, lu, lv, ocw)
                total += n
                t4s += t4
    assert total > 0 and t4s > 0
    print("ocw", ocw, "cells compared", total, "of which clamped at T4", t4s)


def test_field_maxima_at_ocw_40():
    """a box of 81^2 pixels of 255 fills the two fields to their largest values, which the unpack returns whole"""
    img = np.full((200, 200), 255, np.float32)
    S = packed_table(img)
    s, ss, z = query(S, BORDER + 50, BORDER + 60, 81, 81)
    assert (s, ss, z) == (81 * 81 * 255, 81 * 81 * 255 * 255, 0)
    assert s < 1 << SQ and ss < 1 << (NUL - SQ)
    s, ss, z = query(S, BORDER - 40, BORDER - 30, 81, 81)                        # 41 x 51 pixels of the image, the rest border
    assert (s, ss, z) == (41 * 51 * 255, 41 * 51 * 255 * 255, 81 * 81 - 41 * 51)
