"""GPU: the MIMC3_hip_offsets command line (exhaustive-search offsets with peak quality) on TIFF and .GMA files: its [N][10] .GMA is
the Python entry's record (plus u, v) for the same control-point offset and a-priori shifts, and its .txt rows are that record's
points with a peak, in AMPCOR's column order."""
import os
import re
import subprocess

import numpy as np
import pytest

import fileio
from conftest import ROOT, assert_bits_equal, golden_files

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mimc3_amd", "csrc", "MIMC3_hip_offsets")


@pytest.mark.parametrize("args", [[], ["16", "7"]])
def test_offsets_cli_matches_the_python_entry(tmp_path, args):
    from mimc3_amd import api
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mimc3_amd", "csrc"), "cli"])
    z = np.load(golden_files("vmap_small")[0])
    t0, t1 = str(z["t0"]), str(z["t1"])
    d = str(tmp_path)
    fileio.write_tiff(f"{d}/{t0}_i0.tif", z["i0"].astype(np.uint8))
    fileio.write_tiff(f"{d}/{t1}_i1.tif", z["i1"].astype(np.uint8))
    fileio.write_gma(f"{d}/xyuvav.GMA", z["xyuvav"])
    os.makedirs(f"{d}/out")
    p = subprocess.run([CLI, f"{d}/{t0}_i0.tif", f"{d}/{t1}_i1.tif", f"{d}/xyuvav.GMA", f"{d}/out"] + args,
                       env=dict(os.environ, MIMC3_CP_SEED=str(int(z["seed"]))), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = fileio.read_gma(f"{d}/out/offsets_{t0}_{t1}.GMA", np.float32)
    lines = open(f"{d}/out/offsets_{t0}_{t1}.txt").read().splitlines()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", lines[0]).groups()]
    ocw, radius = (int(args[0]), int(args[1])) if args else (15, 15)
    xy = z["xyuvav"]
    with api.Context(0) as ctx:
        ctx.set_images(z["i0"].astype(np.float32), z["i1"].astype(np.float32))
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        want = ctx.match_ncc_full(xy, off, ocw, radius, shift=shift)
    assert got.shape == (xy.shape[0], 10)
    assert_bits_equal(got[:, :8], want, "CLI record")
    assert np.array_equal(got[:, 8], xy[:, 2].astype(np.float32)) and np.array_equal(got[:, 9], xy[:, 3].astype(np.float32))
    ok = want[:, 2] >= -1
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]]).reshape(-1, 8)
    assert rows.shape[0] == ok.sum() > 0
    w = want[ok]
    np.testing.assert_array_equal(rows[:, 0], np.floor(xy[ok, 2]))
    np.testing.assert_array_equal(rows[:, 2], np.floor(xy[ok, 3]))
    np.testing.assert_allclose(rows[:, 1], w[:, 0] + off[0], atol=6e-5)
    np.testing.assert_allclose(rows[:, 3], w[:, 1] + off[1], atol=6e-5)
    np.testing.assert_allclose(rows[:, [4, 5, 6, 7]], w[:, [4, 5, 7, 6]], rtol=1e-5, atol=1e-5)
