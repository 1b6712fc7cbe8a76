"""CPU: the oracle of the exhaustive search beyond +-15 px (mimc3_match_ncc_wide) IS the definition at large R, shown before anything is
compared with it (tests/test_wide.py compares the device with it):
  * a cell is a function of its absolute offset alone: the central 31 x 31 block of an R-20 surface is the R-15 surface, bit for bit;
  * the tail's decisions at R 20 and R 47 -- arg-max, border rule, local maxima and their rank -- against a plain numpy restatement, on
    surfaces with planted ties and a plateau;
  * every fixture of the GPU test holds fitted points, a status -4 and a status -3 point (the counts are stated below);
  * the displaced pair of the GPU test behaves as the test says: found at R 40, out of reach at R 15."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import full_any, tail_from_surface, to_float
from full_multi_common import parity_case, periodic_pair
from wide_common import (CASES, CRAFT_OCW, CRAFT_PERIOD, CRAFT_R, FAR_OCW, FAR_R, FAR_TRUE, body_counts, case_id, far_case, fixture, oracle,
                         status_counts, tail_decisions_py)


# ---- 1. a cell is a function of its absolute offset alone ----
@pytest.mark.parametrize("as_float", [False, True])
def test_central_block_of_a_larger_surface(as_float):
    ocw = 7
    c, shift = parity_case(ocw, 0.03, 20, dimx=4, dimy=3)
    i0, i1 = (to_float(c.i0, 3007), to_float(c.i1, 4007)) if as_float else (c.i0.copy(), c.i1.copy())
    # point 5's box is nulled at both radii: the larger box refuses it
    u, v = int(c.xyuvav[5, 2]) + int(c.offset[0]) + int(shift[5, 0]), int(c.xyuvav[5, 3]) + int(c.offset[1]) + int(shift[5, 1])
    i1[max(v - 27, 0):v + 28, max(u - 27, 0):u + 28] = 0
    r20, _, s20, _ = full_any(i0, i1, c.xyuvav, c.offset, ocw, 20, 0, shift=shift, order=0)
    r15, _, s15, _ = full_any(i0, i1, c.xyuvav, c.offset, ocw, 15, 0, shift=shift, order=0)
    ref20, ref15 = r20[:, 2] == -3, r15[:, 2] == -3
    assert ref20[5] and np.isnan(s20[ref20]).all()
    both = ~ref20 & ~ref15
    assert both.sum() >= 8
    block = s20.reshape(-1, 41, 41)[:, 5:36, 5:36].reshape(-1, 31 * 31)
    assert np.isfinite(block[both]).any()
    assert_bits_equal(block[both], s15[both], "central 31 x 31 block of the R-20 surface vs the R-15 surface")


# ---- 2. the tail's decisions at large R ----
NBUMP = 13


def planted_surface(R, seed, border_peak=False, holes=False):
    """val[x][y]: a low random background (< 0.2) and NBUMP planted maxima of heights 0.5 .. 0.6875 (multiples of 1/64: the fit's f32 sums are exact).  Number 0, the lowest, is a two-cell
    plateau (cells (x, y) and (x, y + 1) equal, 0.125 above the ring around both); the others are symmetric bumps (centre v, its 8
    neighbours v - 0.125: the fit's offset is exactly 0, so a candidate's (du, dv) IS its cell).  Two pairs of bumps are exactly tied, one
    of them at the global maximum.  border_peak: a larger value on the border su = -R.  holes: 2 % of the background is NaN."""
    S = 2 * R + 1
    rng = np.random.default_rng(seed)
    val = (rng.random((S, S)) * 0.2).astype(np.float32)
    if holes:
        val[rng.random((S, S)) < 0.02] = np.nan
    sites = [(x, y) for x in range(3, S - 3, 6) for y in range(3, S - 4, 6)]
    heights = np.float32(0.5) + np.arange(NBUMP, dtype=np.float32) / np.float32(64)
    heights[NBUMP - 2] = heights[NBUMP - 1]                 # the global maximum, twice
    heights[3] = heights[4]                                 # a tie further down
    for j, s in enumerate(rng.choice(len(sites), NBUMP, replace=False)):
        x, y = sites[s]
        val[x - 1:x + 2, y - 1:y + (3 if j == 0 else 2)] = heights[j] - np.float32(0.125)
        val[x, y] = heights[j]
        if j == 0:
            val[x, y + 1] = heights[j]
    if border_peak:
        val[0, S // 2 + 3] = np.float32(0.99)
    return val


@pytest.mark.parametrize("R", [20, 47])
def test_tail_decisions_against_numpy(R):
    S = 2 * R + 1
    surfs = [planted_surface(R, 100 + R), planted_surface(R, 200 + R, border_peak=True), np.full((S, S), np.nan, np.float32),
             planted_surface(R, 300 + R, holes=True)]
    shift = np.array([[0, 0], [4, -3], [1, 1], [-7, 9]], np.int32)
    stack = np.ascontiguousarray(np.stack([s.ravel() for s in surfs]))
    K = 8
    rec, cand = tail_from_surface(stack, shift, R, K)
    statuses = []
    for g, val in enumerate(surfs):
        flat = val.ravel()
        status, k, ranked = tail_decisions_py(val, S * S)
        statuses.append(status)
        if status is None:                                  # the peak is a symmetric bump: (du, dv) is its cell plus the shift
            assert rec[g, 2] == flat[k], f"surface {g}: the peak's value"
            assert (rec[g, 0] - shift[g, 0] + R, rec[g, 1] - shift[g, 1] + R) == divmod(k, S), f"surface {g}: the peak's cell"
        else:
            assert rec[g, 2] == status and np.isnan(rec[g, [0, 1, 3, 4, 5, 6, 7]]).all(), f"surface {g}: status {status}"
        if g != 2:
            # the planted maxima lead the rank; the tied pairs come in ascending k; the plateau is last of them, and there once
            assert len(ranked) > NBUMP
            top = flat[ranked[:NBUMP]]
            assert top[0] == top[1] and ranked[0] < ranked[1] and (np.diff(top) <= 0).all() and top[-1] == np.float32(0.5)
            assert flat[ranked[NBUMP]] < np.float32(0.2)
            assert flat[ranked[NBUMP - 1] + 1] == np.float32(0.5) and ranked[NBUMP - 1] + 1 not in ranked, "the plateau: its lowest k alone"
        else:
            assert ranked == []
        for j in range(K):
            if j < len(ranked):
                assert cand[j, g, 2] == flat[ranked[j]], f"surface {g} slot {j}: value"
                assert (cand[j, g, 0] - shift[g, 0] + R, cand[j, g, 1] - shift[g, 1] + R) == divmod(ranked[j], S), f"surface {g} slot {j}: cell"
            else:
                assert cand[j, g, 2] == -2 and np.isnan(cand[j, g, :2]).all()
    assert statuses == [None, -4, -2, None]
    # a three-cell plateau alone on a nearly flat surface: one slot, at its lowest cell (the fit there leans half a cell towards the
    # plateau; at the middle cell it would add 0, at the highest it would lean back)
    val = np.full((S, S), 0.1, np.float32)
    val[:, :] += (np.random.default_rng(R).random((S, S)) * 0.01).astype(np.float32)
    x, y = R + 5, R - 4
    val[x - 1:x + 2, y - 1:y + 4] = np.float32(0.375)
    val[x, y] = val[x, y + 1] = val[x, y + 2] = np.float32(0.5)
    rec, cand = tail_from_surface(np.ascontiguousarray(val.ravel()[None]), None, R, 2)
    assert cand[0, 0, 2] == np.float32(0.5) and cand[1, 0, 2] < np.float32(0.2), "the plateau fills one slot"
    assert cand[0, 0, 0] == x - R and 0 < cand[0, 0, 1] - (y - R) < 1, "... at its lowest cell"


# ---- 3. the fixtures of the GPU test keep every status ----
# (points with a fit, status -4, status -3, status -2) of the oracle's record, 20 points each; then, of the points that are not -3, those
# without and with an excluded pixel in chip or box: the workgroups of the kernel's clean and of its dirty body
COUNTS = {
    "u8-ocw7-R16": (17, 1, 2, 0, 4, 14),
    "u16-ocw7-R17-noshift": (17, 1, 2, 0, 4, 14),
    "u8-ocw7-R18-swap": (15, 1, 2, 0, 5, 13),
    "u16-ocw7-R47": (18, 1, 1, 0, 12, 7),
    "u8-ocw16-R24": (18, 1, 1, 0, 12, 7),
    "u16-ocw32-R47": (17, 2, 1, 0, 9, 10),
    "u8-ocw40-R39": (15, 4, 1, 0, 9, 10),
    "float-zero-ocw7-R16": (17, 1, 2, 0, 4, 14),
    "float-nan_zero-ocw7-R17-swap": (16, 2, 2, 0, 5, 13),
    "float-m9999_nan-ocw7-R18-noshift": (17, 1, 2, 0, 5, 13),
    "wide-zero-ocw7-R47": (18, 1, 1, 0, 12, 7),
    "wide-nan_zero-ocw16-R24": (17, 2, 1, 0, 12, 7),
    "wide-m9999_nan-ocw32-R47": (16, 3, 1, 0, 9, 10),
    "float-zero-ocw40-R39": (15, 4, 1, 0, 9, 10),
    "float-m9999_nan-ocw16-R24-swap": (18, 1, 1, 0, 12, 7),
}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fixture_statuses(case):
    f = fixture(case)
    rec, surf, nlm = oracle(case)
    fit, n4, n3, n2 = status_counts(rec)
    clean, dirty = body_counts(f, rec)
    print(f'    "{f["what"]}": ({fit}, {n4}, {n3}, {n2}, {clean}, {dirty}),')
    assert fit >= 1 and n4 >= 1 and n3 >= 1
    assert clean >= 3 and dirty >= 3, "one launch holds several workgroups of either body"
    assert rec[f["g4"], 2] == -4 and rec[f["g3"], 2] == -3
    if f["g3box"] is not None:                              # the box rule: the chip is valid, the box is not
        chip = (f["i1"] if f["swap"] else f["i0"])[int(f["xy"][f["g3box"], 3]) - f["ocw"]:, int(f["xy"][f["g3box"], 2]) - f["ocw"]:]
        chip = chip[:2 * f["ocw"] + 1, :2 * f["ocw"] + 1]
        assert rec[f["g3box"], 2] == -3 and (chip.astype(np.float64) < 1e-10).mean() <= 0.8
    assert (fit, n4, n3, n2, clean, dirty) == COUNTS[case_id(case)]
    assert nlm[np.isfinite(rec[:, 0])].min() >= 8, "eight slots fill at every fitted point"


def test_crafted_pair_on_the_oracle():
    """More than 8 local maxima, exact ties among them, and the first-wins peak on the border."""
    p0, p1, xy = periodic_pair(*CRAFT_PERIOD, plateau=False)
    rec, cand, surf, nlm = full_any(p0, p1, xy, (0, 0), CRAFT_OCW, CRAFT_R, 8)
    S = 2 * CRAFT_R + 1
    assert (rec[:, 2] == -4).all() and (nlm > 8).all()
    assert (cand[:, :, 2] == cand[0, :, 2]).all() and np.isfinite(cand).all(), "interior candidates listed at status -4, all tied"
    s = surf.reshape(-1, S, S)
    assert (s[:, 0, CRAFT_R - 11] == cand[0, :, 2]).all(), "the same value on the border su = -R: the arg-max's first"


# ---- 4. what it is for (the CPU half) ----
def test_displaced_pair_on_the_oracle():
    c = far_case()
    far = full_any(c.i0, c.i1, c.xyuvav, (0, 0), FAR_OCW, FAR_R, 0)[0]
    near = full_any(c.i0, c.i1, c.xyuvav, (0, 0), FAR_OCW, 15, 0)[0]
    fitted = np.isfinite(far[:, 0])
    assert fitted.all()
    assert np.hypot(far[:, 0] - FAR_TRUE[0], far[:, 1] - FAR_TRUE[1]).max() < 0.5
    nf = np.isfinite(near[:, 0])
    assert (np.hypot(near[nf, 0] - FAR_TRUE[0], near[nf, 1] - FAR_TRUE[1]) > 15).all()
