"""CPU: what the GPU tests of the coarse-to-fine exhaustive search at any chip size (tests/test_pyramid_chip.py) rest on, without a
device.

  * the two entries and the host query are declared in the header and exported, the Python methods exist;
  * pyramid_chip_path equals the level / kernel table over all classes x ocw 0..81 x mode 0..2;
  * coverage of the fixtures, counted on the oracle's own levels: for each matrix-core kernel and each KCW class some coarser-level
    launch of the parity test's call list holds a point the clean form finishes with a peak, one the masked form finishes with a peak
    and one with no arg-max -- and the stale-peak fixture's four points have no arg-max on level 1 for the four reasons it names;
  * the judge: the comparison the GPU test makes rejects a coarser level's peak moved by one cell;
  * the float case used against pyramid_search_any leaves at most UNDECIDED_CAP of its points undecided, by the oracle alone."""
import os
import re

import numpy as np
import pytest

import pyramid_chip_common as pc
from conftest import ROOT
from pyramid_any_oracle import UNDECIDED_CAP, pyramid_search_any
from pyramid_dn_oracle import pyramid_dn, pyramid_search_dn

SYMBOLS = ("mimc3_match_ncc_pyramid_chip", "mimc3_match_ncc_pyramid_chip_dev", "mimc3_pyramid_chip_path")


def test_symbols_are_declared_and_exported():
    from mimc3_amd import api
    header = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/mimc3_hip.h"
        assert getattr(api._lib, name) is not None
    for name in ("match_ncc_pyramid_chip", "match_ncc_pyramid_chip_dev"):
        assert hasattr(api.Context, name)
    assert hasattr(api, "pyramid_chip_path")
    import inspect
    assert "levels" in inspect.signature(api.Context.full_candidates).parameters


def test_path_query_is_the_table():
    from mimc3_amd import api
    assert api.full_chip_max_ocw() == 80
    for cls, k in pc.CLASS_INDEX.items():
        for ocw in range(0, 82):
            for mode in range(0, 3):
                assert api.pyramid_chip_path(k, ocw, mode) == pc.table_path(cls, ocw, mode), (cls, ocw, mode)
    for k in (-1, 4):
        assert api.pyramid_chip_path(k, 10, 0) == 0
    # the table's own corners, spelled out
    assert [api.pyramid_chip_path(0, o, 0) for o in (7, 10, 40, 80)] == [6, 12, 6, 12]
    assert [api.pyramid_chip_path(0, o, 1) for o in (7, 10)] == [12, 12]
    assert [api.pyramid_chip_path(1, o, m) for o in (7, 10, 16, 80) for m in (0, 1)] == [13] * 8
    assert [api.pyramid_chip_path(2, o, 0) for o in (16, 17)] == [8, 11] and api.pyramid_chip_path(2, 16, 1) == 11
    assert [api.pyramid_chip_path(3, o, 0) for o in (40, 41)] == [9, 11] and api.pyramid_chip_path(3, 40, 1) == 11
    for v in set(pc.table_path(c, o, m) for c in pc.CLASS_INDEX for o in range(1, 81) for m in (0, 1)):
        assert v in pc.PATH_NAME


@pytest.mark.parametrize("cls", ["u8", "u16"])
def test_fixtures_cover_both_forms_in_every_kcw_class(cls):
    """Per KCW class: a clean point with a peak, a masked point with a peak, a point without an arg-max, on some coarser-level launch."""
    seen = {1: set(), 2: set(), 3: set()}
    for ocw in pc.PARITY_OCW + (80,):
        for idx, call in enumerate(pc.parity_calls(cls, ocw)):
            assert call[1].n <= 30
            H, W = call[2].shape
            least = (2 * call[6] + 1) * (1 << (call[8] - 1)) + 45
            assert least <= H <= least + 16 and least <= W <= least + 16, (H, W, least)
            if {"clean", "masked", "none"} <= seen[pc.kcw_class(call[6])]:
                continue                                            # (this KCW class has all three: no more oracle runs for it)
            for lv, kinds in pc.call_kinds(call, pc.expected(cls, ocw, idx)):
                seen[pc.kcw_class(call[6])] |= set(kinds)
    print(cls, {k: sorted(v) for k, v in seen.items()})
    for k in (1, 2, 3):
        assert {"clean", "masked", "none"} <= seen[k], f"{cls}, KCW {k}: only {sorted(seen[k])}"


def test_the_r15_case_has_points_of_its_own():
    for cls in ("u8", "u16"):
        (call,) = pc.parity_calls(cls, 80)
        assert call[6] == 80 and call[7] == 15
        rec, cand, sh, peaks = pc.expected(cls, 80, 0)
        assert (peaks[0] >= 0).any() and (rec[:, 2] >= -1).any()


@pytest.mark.parametrize("cls", ["u8", "u16", "f32", "float"])
def test_stale_fixture_has_the_four_reasons(cls):
    """Level 1 of the second call: no arg-max at the four points, each for its own reason; the first call has an arg-max there."""
    from full_any_common import full_any
    from full_dn_common import full_dn
    from pyramid_any_oracle import pyramid_any
    from pyramid_oracle import _inside
    s = pc.STALE
    i0, i1, xy1, xy2, shift2 = pc.stale_case(cls)
    assert i0.shape == (s["H"], s["W"]) and xy1.shape[0] <= 30
    if cls == "float":
        assert (i0 != np.rint(i0)).any()
        first = pyramid_search_any(i0, i1, xy1, (0, 0), s["ocw"], s["R"], 2)
        l0, l1 = pyramid_any(i0, 2)[1], pyramid_any(i1, 2)[1]
        search = lambda xy, sh: full_any(l0, l1, xy, (0, 0), s["ocw"], s["R"], 0, shift=sh, order=0)[0]
    else:
        first = pyramid_search_dn(i0, i1, xy1, (0, 0), s["ocw"], s["R"], 2)
        l0, l1 = pyramid_dn(i0, 2)[1], pyramid_dn(i1, 2)[1]
        search = lambda xy, sh: full_dn(l0, l1, xy, (0, 0), s["ocw"], s["R"], 0, shift=sh)[0]
    idx = sorted(pc.STALE_POINTS)
    assert first[2][idx].any(axis=1).all(), "the first call leaves a peak other than the centre at the four indices"
    pos = xy2[:, 2:4].astype(np.int64) >> 1
    d = (shift2.astype(np.int64) + 1) >> 1
    ok = _inside(pos, d, s["ocw"], s["R"], *l0.shape)
    assert not ok[0] and pos[0, 0] < s["ocw"] <= xy2[0, 2]                   # the chip leaves level 1, not level 0
    assert not ok[1] and pos[1, 0] + d[1, 0] + s["ocw"] + s["R"] >= l0.shape[1] + pc.PAD      # the box beyond the border
    assert ok[2] and ok[3]
    lxy = np.zeros((2, 6))
    lxy[:, 2:4] = pos[[2, 3]]
    st = search(lxy, np.ascontiguousarray(d[[2, 3]], np.int32))[:, 2]
    assert st.tolist() == [-3.0, -2.0]


def moved_peak(call, exp, level):
    """The oracle's result of a parity call had level `level`'s search found, at every point with an arg-max, the cell one row further
    (sv + 1, or sv - 1 from the last row), every other level's cell as it is -> (record, candidates, shift_out, moved mask)"""
    from full_dn_common import full_dn
    what, c, i0, i1, off, sh, ocw, r, levels, npeaks, swap = call
    pk = exp[3][levels - 1 - level]
    S = 2 * r + 1
    step = np.where(pk % S < S - 1, 1, -1) * (pk >= 0)
    shift_out = exp[2].copy()
    shift_out[:, 1] += (step << level).astype(np.int32)
    rec, cand = full_dn(i0, i1, c.xyuvav, off, ocw, r, npeaks, shift=shift_out, swap=swap)
    return rec, cand, shift_out, pk >= 0


def test_the_judge_rejects_a_peak_moved_by_one_cell():
    compare = pc.compare
    for cls, ocw, k in (("u8", 10, 0), ("u16", 25, 1), ("f32", 45, 3)):
        idx, call = pc.pick(cls, ocw, 3, 4)[k]
        exp = pc.expected(cls, ocw, idx)
        compare(exp[:3], exp[:3], call[0])                                  # (the judge takes the oracle's own result)
        for level in range(1, call[8]):
            rec, cand, sh, moved = moved_peak(call, exp, level)
            assert moved.any()
            np.testing.assert_array_equal(np.abs(sh.astype(np.int64) - exp[2])[moved], [[0, 1 << level]] * int(moved.sum()))
            fit = moved & (exp[0][:, 2] >= -1)
            assert fit.any()
            # (the finer search may find the same match again, 2^level px off the centre of its range: then (du, dv) and the peak stay,
            #  and the SNR, a mean over another window of cells, tells the two apart
            #  -- or the match lies on the range's border or beyond it now: status -4, another peak)
            assert (rec[fit].view(np.uint32) != exp[0][fit].view(np.uint32)).any(axis=1).all(), "a point with a fit keeps its record"
            with pytest.raises(AssertionError):
                compare((rec, cand, sh), exp[:3], call[0])
            with pytest.raises(AssertionError):                             # ... and the record alone gives it away
                compare((rec, cand, exp[2]), exp[:3], call[0])


def test_float_oracle_case_is_decided():
    c, f0, f1, shift, ocw, r, levels = pc.float_oracle_case()
    assert c.n <= 30 and (f0 != np.rint(f0)).any() and np.isnan(f0).any()
    und = pyramid_search_any(f0, f1, c.xyuvav, c.offset, ocw, r, levels, shift=shift)[3]
    print(f"{int(und.sum())} of {c.n} points undecided")
    assert und.mean() <= UNDECIDED_CAP
