"""CPU: the test-side definition of the coarse-to-fine exhaustive search (tests/pyramid_oracle.py) -- its 2 x 2 reduction on hand-built
blocks, L = 1 as the exhaustive search itself, and on a pair moved by (+70, -45) px with no prior: one level at R 15 cannot reach the
motion, three levels recover it.  No GPU."""
import numpy as np

from conftest import assert_bits_equal
from full_search_common import full_search
from mimc3_amd import synth
from pyramid_oracle import BIG, big_case, pyramid_search, reduce2


def test_reduction_on_hand_built_blocks():
    """n = 0..4 non-null pixels, the rounded mean with ties up, and an odd last row / column dropped."""
    blocks = [((0, 0), (0, 0), 0), ((7, 0), (0, 0), 7), ((1, 2), (0, 0), 2), ((1, 0), (0, 4), 3), ((1, 2), (2, 0), 2),
              ((1, 1), (2, 0), 1), ((255, 255), (255, 254), 255), ((3, 4), (4, 4), 4), ((1, 2), (1, 1), 1), ((2, 0), (3, 3), 3)]
    img = np.zeros((3, 2 * len(blocks) + 1), np.float32)
    for j, (top, bot, _) in enumerate(blocks):
        img[0, 2 * j:2 * j + 2] = top
        img[1, 2 * j:2 * j + 2] = bot
    img[2, :] = 200                                    # the odd last row and column never reach level 1
    img[:, -1] = 200
    red = reduce2(img)
    assert red.shape == (1, len(blocks))
    np.testing.assert_array_equal(red[0], [b[2] for b in blocks])
    # a level pixel is null exactly when its whole block is
    rng = np.random.default_rng(3)
    im = rng.integers(0, 256, (64, 66)).astype(np.float32)
    im[rng.random(im.shape) < 0.6] = 0
    r = reduce2(im)
    blk = im.reshape(32, 2, 33, 2)
    np.testing.assert_array_equal(r == 0, (blk != 0).sum(axis=(1, 3)) == 0)
    assert r.max() <= 255


def test_one_level_is_the_exhaustive_search():
    c = synth.make_small(seed=31, shift=(3, -2), ocw=15, h=231, w=243, noise_dn=2, null_frac=0.03, offset=(1, -1))
    shift = np.random.default_rng(1).integers(-3, 4, (c.n, 2)).astype(np.int32)
    rec, sh = pyramid_search(c.i0, c.i1, c.xyuvav, c.offset, 15, 7, 1, shift=shift)
    np.testing.assert_array_equal(sh, shift)
    assert_bits_equal(rec, full_search(c.i0, c.i1, c.xyuvav, c.offset, 15, 7, shift=shift), "L = 1")


def test_three_levels_reach_a_motion_one_level_cannot():
    i0, i1, g = big_case()
    du, dv = BIG["motion"]
    one = full_search(i0, i1, g, (0, 0), BIG["ocw"], 15)
    hit1 = (np.abs(one[:, 0] - du) < 0.05) & (np.abs(one[:, 1] - dv) < 0.05)
    assert hit1.mean() < 0.1 and ((one[:, 2] == -4) | ~hit1).all()
    rec, sh = pyramid_search(i0, i1, g, (0, 0), BIG["ocw"], 15, 3)
    ok = rec[:, 2] >= -1
    hit = ok & (np.abs(rec[:, 0] - du) < 0.05) & (np.abs(rec[:, 1] - dv) < 0.05)
    assert ok.mean() >= 0.9 and hit.sum() >= 0.9 * ok.sum()
    # the level-0 record is the exhaustive search around the chain's shift
    assert_bits_equal(rec, full_search(i0, i1, g, (0, 0), BIG["ocw"], 15, shift=sh), "level 0")
