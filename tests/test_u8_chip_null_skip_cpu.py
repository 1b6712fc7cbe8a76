"""CPU: the chip-null skip of the register-tiled 8-bit kernel restated in numpy at task level (tests/u8_chip_null_skip_common.py: the
flag mask's 19 ballots, the XYC and WNC bodies with their finish) against the per-pixel definition of the six sums, over every cell of
the certain set of every fixture point and over random chips; and the qualifiers of the GPU fixtures of
tests/test_u8_chip_null_skip.py -- each flags exactly the task indices it is named for, counted from its pixels."""
import numpy as np
import pytest

import null_encoding_common as nc
import u8_chip_null_skip_common as cn
import u8_dirty_masks_common as dm

CASES = [(kind, w) for kind in cn.KINDS for w in cn.WINDOWS] + [(kind, "dirty") for kind in cn.T4_KINDS]
SUMS = ("n", "sx", "sy", "sxx", "syy", "sxy")


def u8(a):
    return np.asarray(a).astype(np.int64)


@pytest.fixture(scope="module")
def cases():
    return {(kind, w): cn.make_case(kind, w) for kind, w in CASES}


def random_pairs():
    rng = np.random.default_rng(33)
    for k in range(40):
        chip = rng.integers(1, 256, (cn.CW, cn.CW))
        win = rng.integers(1, 256, (cn.CW + 6, cn.CW + 8))
        chip[rng.random(chip.shape) < (0.002, 0.02, 0.3, 0.9)[k % 4]] = 0
        if k % 8 == 0:
            chip[:, :] = rng.integers(1, 256, chip.shape); chip[rng.integers(0, cn.CW), rng.integers(0, cn.CW)] = 0
        yield chip, win, rng


def test_flag_mask_is_the_definition(cases):
    for chip, _, _ in random_pairs():
        assert cn.flag_mask(chip) == cn.flag_mask_plain(chip)
    for c in cases.values():
        for k in range(12):
            assert cn.flag_mask(u8(c.chip(k))) == cn.flag_mask_plain(u8(c.chip(k)))
    # pad bytes and the idle tail lanes are no nulls: a null-free chip flags nothing
    assert cn.flag_mask(np.full((cn.CW, cn.CW), 7)) == set()


@pytest.mark.parametrize("dirty", [False, True], ids=["xyc", "wnc"])
def test_bodies_on_random_chips(dirty):
    for chip, win, rng in random_pairs():
        if dirty:
            win = win.copy(); win[rng.random(win.shape) < 0.05] = 0
            win[:cn.CW, :cn.CW][(chip == 0) & (rng.random(chip.shape) < 0.5)] = 0     # coincident nulls for cell (0, 0)
        for cx, cy in ((0, 0), (1, 2), (2, 5), (3, 1), (7, 4)):
            got, want = cn.body(chip, win, cx, cy, dirty), cn.plain(chip, win, cx, cy)
            assert all(got[s] == want[s] for s in SUMS), (cx, cy, got, want)


def test_bodies_on_every_fixture_cell(cases):
    for (kind, w), c in cases.items():
        for k in range(12):
            chip, win = u8(c.chip(k)), u8(c.window(k))
            for cx, cy in cn.certain_cells():
                dirty = bool((win[cy:cy + cn.CW, cx:cx + cn.CW] == 0).any())
                got, want = cn.body(chip, win, cx, cy, dirty), cn.plain(chip, win, cx, cy)
                assert all(got[s] == want[s] for s in SUMS), (kind, w, k, cx, cy, got, want)


def test_restatement_sees_the_mutations(cases):
    """The three value-only mutations the GPU tests are run against (profiles/u8_chip_null_skip/README.md) are wrong here as well."""
    def differs(key, cells, dirty, **kw):
        c = cases[key]
        chip, win = u8(c.chip(0)), u8(c.window(0))
        return any(cn.body(chip, win, cx, cy, dirty, **kw)[s] != cn.plain(chip, win, cx, cy)[s] for cx, cy in cells for s in SUMS)
    assert differs(("coincident", "clean"), cn.COINC_CELLS, True, drop_j=True)
    for key in (("tail_lane0", "clean"), ("tail_last", "clean")):
        mask = cn.flag_mask(u8(cases[key].chip(0))) - {18}
        assert differs(key, cn.certain_cells(), False, mask=mask)
    assert differs(("col32", "clean"), cn.certain_cells(), False, pad_nulls=True)


# ---- qualifiers -------------------------------------------------------------------------------------------------------------------
def test_fixtures_hold_what_they_claim(oracle, cases):
    for (kind, w), c in cases.items():
        chip, win = u8(c.chip(0)), u8(c.window(0))
        flags = cn.flag_mask_plain(chip)
        if cn.KINDS.get(kind) is not None:
            assert flags == cn.KINDS[kind], (kind, flags)
        written = win[:-1, :-1]
        if kind in cn.T4_KINDS or w == "dirty" or kind == "coincident":
            assert (written == 0).any()
        else:
            assert not (written == 0).any()
        off, uv = dm.pivots(oracle, c)
        want = oracle.match(c.chip_img, c.win_img, c.xyuvav, c.offset, off, uv, c.ocw)
        assert (want[:, 2] != -3).any()
        assert (want[0, 2] == -3) == (kind == "limit_short"), kind
        if kind in cn.SINGLES or kind in ("tail_lane0", "tail_last", "col32"):
            assert (chip == 0).sum() == 1                        # n drops by exactly one in a clean box
            assert cn.body(chip, win, 12, 2, False)["n"] == cn.NPX - 1 or w == "dirty"
        if kind == "tail_last":
            assert chip[32, 32] == 0
        if kind == "disc":
            assert flags == {1, 2, 3, 4, 5, 10, 11, 12, 13, 14} and (chip[15] == 0).any() and (chip[16] == 0).any()     # across the row-16 boundary
        if kind == "coincident":
            cx0, cy0 = cn.COINC_CELLS[0]
            assert tuple(np.rint(want[0, :2]).astype(int)) == (cx0 - 12, cy0 - 2)     # the peak: the cell and its neighbours are the fit's
            near = ((cx0 - 1, cy0), (cx0 + 1, cy0), (cx0, cy0 - 1), (cx0, cy0 + 1))
            js = {cell: cn.body(chip, win, *cell, True)["J"] for cell in cn.COINC_CELLS + near}
            assert all(js[cell] > 0 for cell in cn.COINC_CELLS)
            # one pixel off in each of the four directions: the neighbours hold the window null, not under a chip null
            for cell in near:
                assert js[cell] == 0 and (win[cell[1]:cell[1] + cn.CW, cell[0]:cell[0] + cn.CW] == 0).any()
        if kind == "extreme_bytes":
            under = {int(win[cy + r, cx + col]) for cx, cy in cn.certain_cells() for r, col in cn.COINC}
            assert set(cn.EXTREME) <= under
        if kind in ("limit_at", "limit_short"):
            assert (chip == 0).sum() == nc.first_invalid_count(cn.NPX) - (1 if kind == "limit_at" else 0)
        if kind == "t4_row":
            assert (np.rint(want[:, 1]) == 1).sum() >= 4 and (chip == 0).any()
        if kind == "t4_col":
            assert (np.rint(want[:, 0]) == 11).sum() >= 4 and (chip == 0).any()
