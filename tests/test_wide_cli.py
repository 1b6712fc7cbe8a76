"""GPU: R beyond 15 on the MIMC3_hip_offsets command line: `... 7 20 1 3 0 1` writes offsets_*, candidates_* and fb_* files that hold
exactly what Context.match_ncc_wide and Context.match_ncc_wide_fb return for the same points, offset and shift, on an 8-bit and on a
16-bit pair; R above mimc3_wide_max_radius(ocw) is refused with the maximum named; levels = 2 with R = 20 is refused naming
"levels = 1"; nothing is written by a refused run."""
import os
import re
import subprocess

import numpy as np
import pytest

import fileio
from conftest import ROOT, assert_bits_equal, golden_files
from full_dn_common import to_dn16

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mimc3_amd", "csrc", "MIMC3_hip_offsets")


def _run(tmp_path, sub, args, dn16=False):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mimc3_amd", "csrc"), "cli"])
    z = np.load(golden_files("vmap_small")[0])
    t0, t1 = str(z["t0"]), str(z["t1"])
    d = str(tmp_path)
    i0, i1 = (to_dn16(z["i0"], 11), to_dn16(z["i1"], 12)) if dn16 else (z["i0"].astype(np.float32), z["i1"].astype(np.float32))
    if not os.path.exists(f"{d}/xyuvav.GMA"):
        fileio.write_tiff(f"{d}/{t0}_i0.tif", i0.astype(np.uint16 if dn16 else np.uint8))
        fileio.write_tiff(f"{d}/{t1}_i1.tif", i1.astype(np.uint16 if dn16 else np.uint8))
        fileio.write_gma(f"{d}/xyuvav.GMA", z["xyuvav"])
    os.makedirs(f"{d}/{sub}")
    p = subprocess.run([CLI, f"{d}/{t0}_i0.tif", f"{d}/{t1}_i1.tif", f"{d}/xyuvav.GMA", f"{d}/{sub}"] + args,
                       env=dict(os.environ, MIMC3_CP_SEED=str(int(z["seed"]))), capture_output=True, text=True, timeout=300)
    return z, i0, i1, t0, t1, f"{d}/{sub}", p


@pytest.mark.parametrize("dn16", [False, True], ids=["8bit", "16bit"])
def test_r20_writes_the_wide_entries_arrays(tmp_path, dn16):
    from mimc3_amd import api
    ocw, R, K = 7, 20, 3
    z, i0, i1, t0, t1, b, p = _run(tmp_path, "b", [str(ocw), str(R), "1", str(K), "0", "1"], dn16=dn16)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    names = [f"fb_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt", f"candidates_{t0}_{t1}.GMA"]
    assert sorted(os.listdir(b)) == sorted(names)
    xy = z["xyuvav"]
    n = xy.shape[0]
    line = open(f"{b}/offsets_{t0}_{t1}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    rec_file = fileio.read_gma(f"{b}/offsets_{t0}_{t1}.GMA", np.float32)
    cand_file = fileio.read_gma(f"{b}/candidates_{t0}_{t1}.GMA", np.float32)
    fb_file = fileio.read_gma(f"{b}/fb_{t0}_{t1}.GMA", np.float32)
    assert rec_file.shape == (n, 10) and cand_file.shape == (K * n, 3) and fb_file.shape == ((1 + K) * n, 4)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)            # (the fixture's dt, as tests/test_full_fb_cli.py)
        w_out, w_cand = ctx.match_ncc_wide(xy, off, ocw, R, K, shift=shift)
        assert ctx.last_path() == "f32g_wide"
        out, cand, fb = ctx.match_ncc_wide_fb(xy, off, ocw, R, K, shift=shift)
    assert_bits_equal(rec_file[:, :8], w_out, "record vs match_ncc_wide")
    assert_bits_equal(cand_file.reshape(K, n, 3), w_cand, "candidates vs match_ncc_wide")
    assert_bits_equal(rec_file[:, :8], out, "record vs match_ncc_wide_fb")
    assert_bits_equal(fb_file.reshape(1 + K, n, 4), fb, "fb vs match_ncc_wide_fb")
    assert np.array_equal(rec_file[:, 8:], xy[:, 2:4].astype(np.float32))
    assert np.isfinite(fb[0, :, 3]).any() and np.isfinite(out[:, 0]).sum() >= n // 4
    # without fb the run takes mimc3_match_ncc_wide: the same two files
    _, _, _, _, _, a, p = _run(tmp_path, "a", [str(ocw), str(R), "1", str(K)], dn16=dn16)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(a)) == sorted(names[1:])
    for name in os.listdir(a):
        assert open(f"{a}/{name}", "rb").read() == open(f"{b}/{name}", "rb").read(), name


def test_radius_above_the_maximum_is_refused(tmp_path):
    from mimc3_amd import api
    _, _, _, _, _, a, p = _run(tmp_path, "a", ["7", "48", "1", "3", "0", "1"])
    assert p.returncode != 0 and str(api.wide_max_radius(7)) in p.stderr and "47" in p.stderr
    assert os.listdir(a) == []
    _, _, _, _, _, b, p = _run(tmp_path, "b", ["40", "40"])
    assert p.returncode != 0 and str(api.wide_max_radius(40)) in p.stderr and "39" in p.stderr
    assert os.listdir(b) == []


def test_wide_radius_on_a_pyramid_is_refused(tmp_path):
    _, _, _, _, _, a, p = _run(tmp_path, "a", ["7", "20", "2"])
    assert p.returncode != 0 and "levels = 1" in p.stderr
    assert os.listdir(a) == []
