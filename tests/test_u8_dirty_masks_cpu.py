"""CPU: the byte-mask helper of the register-tiled kernel's masked bodies (match_px_kernel.hip: nzff, PxU8::task), restated in numpy
instruction by instruction, against the plain per-byte definition; and the qualifiers of the GPU fixtures of
tests/test_u8_dirty_masks.py -- each really holds the cell kinds it is there for, counted from its pixels."""
import numpy as np
import pytest

import null_encoding_common as nc
import u8_dirty_masks_common as dm

OCW = (7, 16, 40)


@pytest.fixture(scope="module")
def dwords():
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 16, 20000).astype(np.uint32)                # random dwords with random bytes zeroed
    keep = sum((((bits >> np.uint32(k)) & np.uint32(1)) * np.uint32(0xFF)) << np.uint32(8 * k) for k in range(4))
    sparse = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32) & keep
    return np.concatenate([dm.edge_dwords(), rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32), sparse])


def test_helper_is_exact(dwords):
    """Every byte value at every byte position beside neighbours 0, 1, 0x7f, 0x80, 0xff (carries, borrows and the saturation of the
    half-word add all act between neighbours), and random dwords: the mask is the definition's, with no false alarm."""
    assert len(dm.edge_dwords()) == 4 * 256 * 125
    assert np.array_equal(dm.nzff(dwords), dm.nzff_plain(dwords))


def test_helper_restatement_sees_the_mutations(dwords):
    """The two value-only mutations that the GPU tests are run against (profiles/u8_dirty_masks/README.md) are wrong in the
    restatement as well: a selector with two bytes swapped, and a half-word addend without its shift."""
    assert not np.array_equal(dm.nzff(dwords, sel=0x0B0A0908), dm.nzff_plain(dwords))
    assert not np.array_equal(dm.nzff(dwords, shift_hi=0x007F007F), dm.nzff_plain(dwords))


@pytest.mark.parametrize("chip_mask", [None, 0xFFFFFFFF, 0x000000FF, 0x00FFFFFF], ids=["derived", "full", "last1", "last3"])
def test_body_sums(dwords, chip_mask):
    """The sums of a dword task as the bodies form them -- masked chip bytes, sx as their dot product with ones, the pixel count as a
    population count in units of eight -- against the definition, for window and chip dwords from the same value set."""
    bw = dwords
    a = np.roll(dwords, 7777)
    if chip_mask is not None:
        a = (a | np.uint32(0x01010101)) & np.uint32(chip_mask)          # a null-free chip row: pad bytes 0, every other byte valid
    got, want = dm.body_sums(a, bw, chip_mask), dm.plain_sums(a, bw, chip_mask)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- qualifiers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocw", OCW)
def test_fixtures_hold_what_they_claim(oracle, ocw):
    for lift in (0, 200):
        cases = {kind: dm.make_case(ocw, kind, lift) for kind in dm.KINDS}
        want = {}
        for kind, c in cases.items():
            off, uv = dm.pivots(oracle, c)
            want[kind] = oracle.match(c.chip_img, c.win_img, c.xyuvav, c.offset, off, uv, ocw)
            assert want[kind][0, 2] != -3, (kind, "point 0 is invalid")
            assert c.win_img.max() <= 255 + lift and (lift == 0 or c.win_img[c.win_img > 0].min() > 200)
        kinds = {kind: dm.cell_kinds(c, 0) for kind, c in cases.items()}
        allk = {kind: [dm.cell_kinds(c, k) for k in range(12)] for kind, c in cases.items() if kind in ("single_phases", "box_sides")}
        # single nulls: every (box phase, null phase) pair over the fixture's points, boxes with exactly one null
        ph = set().union(*[k["phases"] for k in allk["single_phases"]])
        assert ph == {(b, z) for b in range(4) for z in range(4)}
        assert kinds["single_phases"]["min_valid"] >= (2 * ocw + 1) ** 2 - 4 and kinds["single_phases"]["dirty"] > 0
        # around the box: a null under a pad byte, and one pixel outside on each side, in some cell of the certain set
        bs = kinds["box_sides"]
        assert bs["pad"] > 0 and bs["left"] > 0 and bs["right"] > 0 and bs["above"] > 0 and bs["below"] > 0
        # carries: the neighbours are in place
        c = cases["carry"]
        w = c.window(0)
        zy, zx = np.argwhere(w[:-1, :-1] == 0).T
        pairs = {(int(w[y, x - 1]) - lift, int(w[y, x + 1]) - lift) for y, x in zip(zy, zx)}
        assert pairs == set(dm.NEIGHBOURS)
        # the blob's edge: clean and dirty cells in one point's certain set
        assert kinds["blob_edge"]["clean"] >= 9 and kinds["blob_edge"]["dirty"] >= 9
        # T4: the climbs end where their last scan covered the never-written row / column, with window nulls in those boxes
        assert (np.rint(want["t4_row"][:, 1]) == 1).sum() >= 6 and kinds["t4_row"]["dirty"] > 0
        assert (np.rint(want["t4_col"][:, 0]) == 11).sum() >= 6 and kinds["t4_col"]["dirty"] > 0
        # nulls on both sides
        c = cases["both_sides"]
        assert (c.chip(0) == 0).sum() == 4 and kinds["both_sides"]["dirty"] > 0
        # one valid pixel in a box; point 0 one invalid pixel short of the 80 % rule, the next one tips it
        c = cases["one_valid_limit"]
        assert kinds["one_valid_limit"]["min_valid"] == 1
        Dx2, Dy2, _ = dm.geometry(ocw)
        assert int((c.window(0) == 0).sum()) == nc.first_invalid_count(Dx2 * Dy2) - 1
