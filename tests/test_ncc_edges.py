"""NCC cells at f32 rounding boundaries (tests/golden/ncc_edge_*.npz, tests/ncc_edge_common.py).

Every matcher rounds the reference's f64 value Qd = num / sqrt(P) of a cell to f32.  The matrix-core kernel takes a faster f64 quotient
and redoes a cell with the reference's operations only when that quotient lies within 2^13 f64 ulps of an f32 rounding midpoint
(match_mx_kernel.hip); the other kernels must round sqrt and the division correctly.  Random textures almost never put a
peak or a peak neighbour within a few ulps of a midpoint: these fixtures do, at every matrix-core chip size, in the clean, the
window-null and the chip-null form.

CPU: the fixtures' own claims (d recomputed with numpy from exact integer sums), the port oracle, the exhaustive-search oracle and the
compiled reference on them.  GPU: every DLC path and the exhaustive search against the oracles, bit for bit."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal
from full_search_common import assert_records_match, full_search
from ncc_edge_common import NEIGHBOURS, T_D, T_FORM, T_POINT, T_ROLE, cell_sums, fit, fixture_paths, load, midpoint_distance, qd

PATHS = fixture_paths()
IDS = [os.path.basename(p)[len("ncc_edge_"):-4] for p in PATHS]
MODES = ("auto", "u8px", "u16", "f32", "general")


@pytest.fixture(scope="module", params=PATHS, ids=IDS)
def fx(request):
    return load(request.param)


def pivots(f, g):
    return f["piv_uv"][f["piv_off"][g]:f["piv_off"][g + 1]]


def expected(f):
    """-> ([N][3] f32: the fit and the peak value from numpy alone, with the peak on (0, 0)), the target cells' f32 values"""
    ocw, off = f["ocw"], f["offset"]
    n = f["xyuvav"].shape[0]
    want = np.empty((n, 3), np.float32)
    for g in range(n):
        n9 = [np.float32(qd(cell_sums(f["i0"], f["i1"], f["xyuvav"], off, ocw, g, c - 1, r - 1))) for r in range(3) for c in range(3)]
        du, dv = fit(n9, 0, 0)
        want[g] = (du, dv, n9[4])
    return want


# ---- CPU: the fixtures' claims ---------------------------------------------------------------------------------------------------------
def test_fixture_content():
    """Recompute every target's d from the images (numpy int64 sums, the f64 formula) and check the content the fixtures promise."""
    assert PATHS, "no tests/golden/ncc_edge_*.npz"
    assert sum(os.path.getsize(p) for p in PATHS) <= 1 << 20
    all_d, sizes = [], set()
    for p in PATHS:
        f = load(p)
        ocw, t, n = f["ocw"], f["targets"], f["xyuvav"].shape[0]
        sizes.add(ocw)
        assert np.array_equal(t[:, T_POINT], np.arange(n)) and len(f["piv_off"]) == n + 1
        for row in t:
            g, su, sv, role, form, d = (int(v) for v in row)
            assert (su, sv) == ((0, 0) if role == 0 else NEIGHBOURS[role - 1])
            assert midpoint_distance(qd(cell_sums(f["i0"], f["i1"], f["xyuvav"], f["offset"], ocw, g, su, sv))) == d, (f["name"], g)
            u0, v0 = int(f["xyuvav"][g, 2]), int(f["xyuvav"][g, 3])
            uc, vc = u0 + int(f["offset"][0]), v0 + int(f["offset"][1])
            R = f["radius"]
            chip = f["i0"][v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1]
            win = f["i1"][vc - ocw - R - 1:vc + ocw + R + 2, uc - ocw - R - 1:uc + ocw + R + 2]
            box = f["i1"][vc + sv - ocw:vc + sv + ocw + 1, uc + su - ocw:uc + su + ocw + 1]
            assert (chip == 0).any() == (form == 2) and (win == 0).any() == (form == 1), (f["name"], g)
            assert form != 1 or (box == 0).any()                 # the target cell itself reads window nulls
            piv = pivots(f, g)
            assert np.abs(piv).max(axis=1).argmax() == len(piv) - 1     # the last pivot has the largest extent (window size)
        forms = set(t[:, T_FORM].tolist())
        assert forms == {0, 1, 2}, (ocw, forms)
        assert {0} < set(t[:, T_ROLE].tolist()), ocw                   # peaks and neighbours
        far = [g for g in range(n) if np.abs(pivots(f, g)).max() >= 3 and t[g, T_ROLE] == 0]
        assert far, f"ocw {ocw}: no peak reached by a climb of 3 or more scans"
        all_d.append(t[:, T_D])
    assert {7, 16, 40} <= sizes
    d = np.concatenate(all_d)
    near = d[(np.abs(d) >= 1) & (np.abs(d) <= 4)]
    assert near.size >= 128 and (near > 0).sum() >= 32 and (near < 0).sum() >= 32, (near.size, (near > 0).sum())
    assert ((np.abs(d) >= 5) & (np.abs(d) <= 64)).any()
    for edge in (1 << 13, 1 << 14):
        assert (np.abs(np.abs(d) - edge) <= 16).sum() >= 2, edge


def test_port_oracle_on_fixtures(oracle, fx):
    """The port oracle's DLC match: the peak value is the f32 rounding of the (0, 0) cell's Qd and the fit reads the target's 3 x 3
    block (du, dv bit for bit from the numpy fit of the numpy cells)."""
    got = oracle.match(fx["i0"], fx["i1"], fx["xyuvav"], fx["offset"], fx["piv_off"], fx["piv_uv"], fx["ocw"])
    assert_bits_equal(got, expected(fx), fx["name"])


def test_full_search_oracle_on_fixtures(fx):
    """The exhaustive-search oracle: its arg-max is the (0, 0) cell, its record's du, dv, peak are the numpy fit and value."""
    R, S = fx["radius"], 2 * fx["radius"] + 1
    out, peak = full_search(fx["i0"], fx["i1"], fx["xyuvav"], fx["offset"], fx["ocw"], R, with_peak=True)
    assert (peak == R * S + R).all()
    assert_bits_equal(out[:, :3], expected(fx), fx["name"])


def test_reference_on_fixtures(oracle, reference, fx):
    """The compiled reference equals the port oracle bit for bit, both directions."""
    a = (fx["xyuvav"], fx["offset"], fx["piv_off"], fx["piv_uv"], fx["ocw"])
    for i0, i1, s in ((fx["i0"], fx["i1"], 1), (fx["i1"], fx["i0"], -1)):
        xy, off, po, uv, ocw = a
        assert_bits_equal(reference.match(i0, i1, xy, s * off, po, s * uv, ocw), oracle.match(i0, i1, xy, s * off, po, s * uv, ocw),
                          f"{fx['name']} {'swapped' if s < 0 else 'forward'}")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_dlc_paths_on_fixtures(api, oracle, fx, mode):
    """Every DLC path, both directions, bit for bit against the port oracle ("auto": the matrix-core kernel's guarded finish)."""
    a = (fx["xyuvav"], fx["offset"], fx["piv_off"], fx["piv_uv"], fx["ocw"])
    xy, off, po, uv, ocw = a
    with api.Context(0) as ctx:
        ctx.set_images(fx["i0"], fx["i1"])
        ctx.set_path(mode)
        got = ctx.matching_ncc_dlc_2(xy, off, po, uv, ocw)
        if mode == "auto":
            assert ctx.last_path() == "u8_mfma"
        assert_bits_equal(got, oracle.match(fx["i0"], fx["i1"], xy, off, po, uv, ocw), f"{fx['name']} {mode}")
        sw = ctx.matching_ncc_dlc_2(xy, -off, po, -uv, ocw, swap=True)
        assert_bits_equal(sw, oracle.match(fx["i1"], fx["i0"], xy, -off, po, -uv, ocw), f"{fx['name']} {mode} swapped")


@pytest.mark.gpu
def test_mx_null_forms_on_fixtures():
    """The matrix-core window-null and general forms switched on (a subprocess: the switches are read once per process) on every
    fixture: the null-ridden points' target cells then take those forms' finish."""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
        from conftest import assert_bits_equal
        from ncc_edge_common import fixture_paths, load
        from mimc3_amd import api
        from oracle import oracle as orc
        o = orc.Oracle("port")
        with api.Context(0) as ctx:
            for p in fixture_paths():
                f = load(p)
                xy, off, po, uv, ocw = f["xyuvav"], f["offset"], f["piv_off"], f["piv_uv"], f["ocw"]
                ctx.set_images(f["i0"], f["i1"])
                got = ctx.matching_ncc_dlc_2(xy, off, po, uv, ocw)
                assert ctx.last_path() == "u8_mfma"
                assert_bits_equal(got, o.match(f["i0"], f["i1"], xy, off, po, uv, ocw), f["name"])
                sw = ctx.matching_ncc_dlc_2(xy, -off, po, -uv, ocw, swap=True)
                assert_bits_equal(sw, o.match(f["i1"], f["i0"], xy, -off, po, -uv, ocw), f["name"] + " swapped")
    """ % (ROOT, ROOT))
    env = dict(os.environ, MIMC3_MX_GEN="1", MIMC3_MX_WN="1")
    subprocess.check_call([sys.executable, "-c", code], env=env, timeout=300)


@pytest.mark.gpu
def test_full_search_on_fixtures(api, fx):
    """The exhaustive search at the fixtures' radius, both directions and the _dev twin, against the exhaustive-search oracle."""
    from hipmem import DevArray
    xy, off, ocw, R = fx["xyuvav"], fx["offset"], fx["ocw"], fx["radius"]
    n = xy.shape[0]
    with api.Context(0) as ctx:
        ctx.set_images(fx["i0"], fx["i1"])
        got = ctx.match_ncc_full(xy, off, ocw, R)
        assert ctx.last_path() == "u8_mfma_full"
        assert_records_match(got, full_search(fx["i0"], fx["i1"], xy, off, ocw, R), fx["name"])
        sw = ctx.match_ncc_full(xy, -off, ocw, R, swap=True)
        assert_records_match(sw, full_search(fx["i0"], fx["i1"], xy, -off, ocw, R, swap=True), fx["name"] + " swapped")
        d_xy, d_out = DevArray(src=np.ascontiguousarray(xy)), DevArray((n, 8), np.float32)
        ctx.match_ncc_full_dev(d_xy.ptr, n, off, ocw, R, d_out.ptr)
        assert_bits_equal(d_out.numpy(), got, fx["name"] + " _dev")
