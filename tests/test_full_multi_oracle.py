"""CPU: the test-side oracle of the exhaustive search with candidates (tests/full_multi_oracle.c) against the exhaustive search's own
oracle (its [N][8] record, bit for bit in all 8 columns), against its own consequences (candidate 0 is the record's fit; the slot
statuses), and against a brute-force Python restatement of the local-maximum rule and its rank on small cases; and the C ABI's
two new symbols."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal
from full_multi_common import filled_fraction, full_multi, parity_case, ranked_local_maxima_py, surface_py
from full_search_common import full_search


@pytest.mark.parametrize("ocw,null_frac,radius", [(7, 0.0, 1), (7, 0.15, 7), (15, 0.03, 7), (16, 0.15, 15), (30, 0.03, 7), (40, 0.0, 15)])
def test_record_equals_the_exhaustive_search_oracle(ocw, null_frac, radius):
    """Same statements in the same order: all 8 columns bit for bit, both directions; and where the record has a fit, candidate 0
    is its columns 0-2."""
    c, shift = parity_case(ocw, null_frac, radius)
    for swap in (False, True):
        sgn = -1 if swap else 1
        out, cand = full_multi(c.i0, c.i1, c.xyuvav, sgn * c.offset, ocw, radius, 3, shift=sgn * shift, swap=swap)
        assert_bits_equal(out, full_search(c.i0, c.i1, c.xyuvav, sgn * c.offset, ocw, radius, shift=sgn * shift, swap=swap), f"record swap {swap}")
        fit = out[:, 2] >= -1
        assert fit.sum() > c.n // 2
        assert_bits_equal(cand[0][fit], out[fit, :3], "candidate 0 vs the record")
        if radius == 1:
            assert (cand[1:, :, 2] <= -2).all() and np.isnan(cand[1:, :, :2]).all()      # one interior cell: at most one candidate


@pytest.mark.parametrize("radius", [1, 2, 7])
@pytest.mark.parametrize("null_frac", [0.0, 0.15])
def test_local_maxima_and_rank_against_brute_force(null_frac, radius):
    """ocw 7: every point's whole ranked list of local maxima (k in order) equals the Python restatement's on a surface computed in
    numpy, and the candidates' NCC are that surface's cells."""
    c, shift = parity_case(7, null_frac, radius, dimx=4, dimy=3)
    cap = (2 * radius - 1) ** 2
    out, cand, nlm, lmk = full_multi(c.i0, c.i1, c.xyuvav, c.offset, 7, radius, 8, shift=shift, with_counts=True, lmcap=cap)
    seen = 0
    for g in range(c.n):
        u0, v0 = int(c.xyuvav[g, 2]), int(c.xyuvav[g, 3])
        val = surface_py(c.i0, c.i1, u0, v0, u0 + c.offset[0] + shift[g, 0], v0 + c.offset[1] + shift[g, 1], 7, radius)
        if val is None:
            assert out[g, 2] == -3 and (cand[:, g, 2] == -3).all() and np.isnan(cand[:, g, :2]).all()
            continue
        want = ranked_local_maxima_py(val)
        assert nlm[g] == len(want)
        assert lmk[g, :len(want)].tolist() == want and (lmk[g, len(want):] == -1).all()
        for j in range(8):
            if j < len(want):
                assert cand[j, g, 2].view(np.uint32) == val.reshape(-1)[want[j]].view(np.uint32)
            else:
                assert cand[j, g, 2] == -2 and np.isnan(cand[j, g, :2]).all()
        seen += len(want)
    assert seen >= (1 if radius == 1 else c.n)
    if radius == 1:
        assert nlm.max() <= 1


def test_status_slots():
    """-3: every slot (NaN, NaN, -3); -2 (a flat chip: no finite cell): every slot (NaN, NaN, -2); -4: the interior local maxima."""
    from full_multi_common import STATUS_R, status_case
    i0, i1, xy = status_case()
    out, cand, nlm = full_multi(i0, i1, xy, (0, 0), 7, STATUS_R, 4, with_counts=True)
    assert out[0, 2] == -3 and (cand[:, 0, 2] == -3).all() and np.isnan(cand[:, 0, :2]).all()
    assert out[1, 2] == -2 and (cand[:, 1, 2] == -2).all() and np.isnan(cand[:, 1, :2]).all() and nlm[1] == 0
    assert out[2, 2] == -4 and nlm[2] >= 4 and (cand[:, 2, 2] >= -1).all() and np.isfinite(cand[:, 2, :2]).all()
    assert (np.abs(cand[:, 2, :2]) < STATUS_R).all()             # interior cells' fits


def test_random_textures_fill_the_slots():
    """The parity fixtures must not pass vacuously: with R >= 7, at least 90 % of the points with a peak have all 8 slots filled."""
    for ocw, null_frac, radius in ((7, 0.15, 7), (16, 0.0, 7), (32, 0.03, 15), (40, 0.15, 7)):
        c, shift = parity_case(ocw, null_frac, radius)
        out, cand = full_multi(c.i0, c.i1, c.xyuvav, c.offset, ocw, radius, 8, shift=shift)
        assert filled_fraction(out, cand) >= 0.9, (ocw, null_frac, radius)


def test_decoy_fixture_on_the_oracle_chain(oracle):
    """The decoy fixture does what it is built for, on the oracle's search and the oracle's chain: with the single best peak the final
    field is more than 1 px wrong at the four decoy points (it is the decoy, 15 px away); with 4 candidates per point clustering and
    the neighbourhood pick the truth, within 0.1 px.  The other points stay within 0.1 px either way."""
    from full_multi_common import DECOY_OCW, DECOY_R, decoy_case, decoy_errors, oracle_postprocess
    c, shift, pts = decoy_case()
    mps = float(np.float32(c.xyuvav[1, 0] - c.xyuvav[0, 0]))
    for npeaks in (1, 4):
        out, cand = full_multi(c.i0, c.i1, c.xyuvav, c.offset, DECOY_OCW, DECOY_R, npeaks, shift=shift)
        assert (out[pts, 2] > 0.9).all() and (np.hypot(out[pts, 0] - 3, out[pts, 1] + 2) > 10).all()      # the record: the decoy
        at, rest = decoy_errors(oracle_postprocess(oracle, cand, c.xyuvav, c.dimx, c.dimy, mps, c.dt, c.mpp), pts)
        print(f"npeaks {npeaks}: error at the decoy points {at.tolist()}, largest elsewhere {rest}")
        assert rest < 0.1
        assert (at > 1.0).all() if npeaks == 1 else (at < 0.1).all()


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for name in ("mimc3_match_ncc_full_multi", "mimc3_match_ncc_full_multi_dev"):
        assert hasattr(lib, name), f"{name} not exported"
    from mimc3_amd import api
    assert callable(api.Context.match_ncc_full_multi) and callable(api.Context.match_ncc_full_multi_dev)
