"""GPU: the peaks argument of the MIMC3_hip_offsets command line: peaks=1 writes byte-identical files to a run without the argument,
peaks=3 also writes candidates_<t0>_<t1>.GMA -- [3 N][3], pass-major, equal to the oracle's candidates for the offset the run
reports -- and peaks > 1 with levels > 1 is refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import fileio
from conftest import ROOT, assert_bits_equal, golden_files
from full_multi_common import full_multi

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mimc3_amd", "csrc", "MIMC3_hip_offsets")


def _run(tmp_path, sub, args):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mimc3_amd", "csrc"), "cli"])
    z = np.load(golden_files("vmap_small")[0])
    t0, t1 = str(z["t0"]), str(z["t1"])
    d = str(tmp_path)
    if not os.path.exists(f"{d}/xyuvav.GMA"):
        fileio.write_tiff(f"{d}/{t0}_i0.tif", z["i0"].astype(np.uint8))
        fileio.write_tiff(f"{d}/{t1}_i1.tif", z["i1"].astype(np.uint8))
        fileio.write_gma(f"{d}/xyuvav.GMA", z["xyuvav"])
    os.makedirs(f"{d}/{sub}")
    p = subprocess.run([CLI, f"{d}/{t0}_i0.tif", f"{d}/{t1}_i1.tif", f"{d}/xyuvav.GMA", f"{d}/{sub}"] + args,
                       env=dict(os.environ, MIMC3_CP_SEED=str(int(z["seed"]))), capture_output=True, text=True, timeout=300)
    return z, t0, t1, f"{d}/{sub}", p


def test_peaks_1_writes_todays_files(tmp_path):
    _, t0, t1, a, p = _run(tmp_path, "a", ["16", "7"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, _, b, p = _run(tmp_path, "b", ["16", "7", "1", "1"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == [f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt"]
    for name in os.listdir(a):
        assert open(f"{a}/{name}", "rb").read() == open(f"{b}/{name}", "rb").read(), name


def test_peaks_3_writes_the_candidates(tmp_path):
    from mimc3_amd import api
    z, t0, t1, a, p = _run(tmp_path, "a", ["16", "7"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, _, b, p = _run(tmp_path, "b", ["16", "7", "1", "3"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for name in (f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt"):
        assert open(f"{a}/{name}", "rb").read() == open(f"{b}/{name}", "rb").read(), name
    got = fileio.read_gma(f"{b}/candidates_{t0}_{t1}.GMA", np.float32)
    xy = z["xyuvav"]
    n = xy.shape[0]
    assert got.shape == (3 * n, 3)
    line = open(f"{b}/offsets_{t0}_{t1}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    i0, i1 = z["i0"].astype(np.float32), z["i1"].astype(np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
    want_out, want = full_multi(i0, i1, xy, off, 16, 7, 3, shift=shift)
    assert_bits_equal(got.reshape(3, n, 3), want, "CLI candidates")
    assert (want[0, :, 2] >= -1).sum() > n // 2


def test_peaks_on_a_pyramid_are_refused(tmp_path):
    _, _, _, a, p = _run(tmp_path, "a", ["16", "7", "2", "2"])
    assert p.returncode != 0 and "levels = 1" in p.stderr
    assert os.listdir(a) == []
