"""CPU: the test-side oracle of the exhaustive search (tests/full_search_oracle.c) pinned to the DLC oracle (oracle/mimc3_oracle.c,
Oracle.match) where the two must agree, and its rules on hand-made surfaces.  No GPU."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_search_common import full_search
from mimc3_amd import synth


@pytest.mark.parametrize("ocw,radius,swap", [(7, 7, False), (7, 4, True), (15, 6, False)])
def test_peak_and_fit_agree_with_the_dlc_matcher(oracle, ocw, radius, swap):
    """On a null-free pair, give every point a ONE-pivot list placed at the exhaustive peak s.  The DLC climb starts there and scans
    the 3x3 block around it; the exhaustive peak is the first maximum in the same u-outer, v-inner order over a range that holds that
    block, so every cell the scan visits before the peak is strictly lower and none after it is higher: the climb stays, its maximum
    is the peak's value, and its fit reads the same 3x3 block.  The DLC window (|s| + ocw + 2 around uv0 + offset) holds every box of
    that block away from its never-written last row and column, and outside the image both sides read zeros.  So columns 0-2 of the
    exhaustive record are the DLC output bit for bit: du, dv = fit + s, and the peak NCC."""
    c = synth.make_small(seed=61 + ocw, shift=(3, -2), angle_deg=30.0, ocw=ocw, h=2 * ocw + 150, w=2 * ocw + 160, dimx=7, dimy=6,
                         noise_dn=2, null_frac=0.0, offset=(1, -1))
    i0, i1 = (c.i1, c.i0) if swap else (c.i0, c.i1)
    off = -c.offset if swap else c.offset
    rec, peak = full_search(i0, i1, c.xyuvav, off, ocw, radius, with_peak=True)
    ok = rec[:, 2] >= -1.0
    assert ok.sum() >= c.n // 2, f"only {ok.sum()} of {c.n} points have an interior peak"
    S = 2 * radius + 1
    piv = np.stack([peak // S - radius, peak % S - radius], axis=1).astype(np.int32)[ok]
    piv_off = np.arange(ok.sum() + 1, dtype=np.int64)
    dlc = oracle.match(i0, i1, c.xyuvav[ok], off, piv_off, piv, ocw)
    assert_bits_equal(rec[ok, :3], dlc, "exhaustive oracle vs DLC oracle")


def test_status_rules():
    """-3 for a window more than 80 % null, -2 for a flat chip (no finite cell), -4 for a peak on the border."""
    H = W = 96
    i0 = synth.texture(H, W, 3, sigma=3.0)                    # smooth: the NCC climbs toward the true offset
    i1 = np.roll(i0, (0, 5), axis=(0, 1)).copy()           # i1 = i0 moved by +5 px in u
    xy = np.zeros((3, 6))
    xy[:, 2:4] = [[40, 40], [48, 48], [56, 40]]
    i1_null = i1.copy()
    i1_null[20:80, 20:80] = 0                               # point 0's search box is > 80 % null
    rec = full_search(i0, i1_null, xy[:1], (0, 0), 7, 3)
    assert rec[0, 2] == -3 and np.isnan(rec[0, [0, 1, 3, 4, 5, 6, 7]]).all()
    flat = i0.copy()
    flat[48 - 7:48 + 8, 48 - 7:48 + 8] = 9                  # point 1's chip is flat: every cell 0 / 0
    assert full_search(flat, i1, xy[1:2], (0, 0), 7, 3)[0, 2] == -2
    rec = full_search(i0, i1, xy[2:3], (0, 0), 7, 3)        # the true offset +5 lies beyond R = 3: the peak sits on the border
    assert rec[0, 2] == -4 and np.isnan(rec[0, 0])
    rec = full_search(i0, i1, xy[2:3], (0, 0), 7, 6)        # ... and inside R = 6
    assert rec[0, 2] > 0.99 and abs(rec[0, 0] - 5) < 0.05 and abs(rec[0, 1]) < 0.05
    assert rec[0, 4] > 1 and rec[0, 5] < 0 and rec[0, 7] < 0   # a sharp maximum: SNR > 1, negative curvature


def test_shift_moves_the_search_centre():
    """shift = k on a pair whose i1 is moved by k gives the record of shift = 0 on the unmoved pair: the same cells, peak, fit and
    quality columns bit for bit; du, dv carry k on top (fit + (s + k) in f32, so within rounding of base + k)."""
    c = synth.make_small(seed=9, shift=(2, 1), ocw=7, null_frac=0.03)
    k = np.array([4, -3])
    i1m = np.zeros_like(c.i1)
    i1m[max(k[1], 0):c.i1.shape[0] + min(k[1], 0), max(k[0], 0):c.i1.shape[1] + min(k[0], 0)] = \
        c.i1[max(-k[1], 0):c.i1.shape[0] + min(-k[1], 0), max(-k[0], 0):c.i1.shape[1] + min(-k[0], 0)]
    base = full_search(c.i0, c.i1, c.xyuvav, (0, 0), 7, 5)
    moved = full_search(c.i0, i1m, c.xyuvav, (0, 0), 7, 5, shift=np.tile(k, (c.n, 1)))
    good = base[:, 2] >= -1
    assert good.sum() > c.n // 2
    assert_bits_equal(moved[good, 2:], base[good, 2:], "shifted")
    assert np.allclose(moved[good, :2] - k, base[good, :2], rtol=0, atol=1e-5)
    assert_bits_equal(moved[~good], base[~good], "shifted, no fit")
