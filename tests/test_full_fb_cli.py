"""GPU: the fb argument of the MIMC3_hip_offsets command line: fb=1 also writes fb_<t0>_<t1>.GMA -- [(1 + K) N][4], plane-major, equal to
match_ncc_full_fb's array for the offset the run reports -- on an 8-bit pair and on a 16-bit pair with peaks=3; fb=0 writes
byte-identical files to a run without the argument; fb=1 with levels=2 is refused and nothing is written."""
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


@pytest.mark.parametrize("dn16,peaks", [(False, 1), (True, 3)])
def test_fb_1_writes_the_entrys_array(tmp_path, dn16, peaks):
    from mimc3_amd import api
    z, i0, i1, t0, t1, b, p = _run(tmp_path, "b", ["16", "7", "1", str(peaks), "0", "1"], dn16=dn16)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    K = peaks if peaks != 1 else 0
    names = [f"fb_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt"] + ([f"candidates_{t0}_{t1}.GMA"] if K else [])
    assert sorted(os.listdir(b)) == sorted(names)
    xy = z["xyuvav"]
    n = xy.shape[0]
    line = open(f"{b}/offsets_{t0}_{t1}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    fb_file = fileio.read_gma(f"{b}/fb_{t0}_{t1}.GMA", np.float32)
    rec_file = fileio.read_gma(f"{b}/offsets_{t0}_{t1}.GMA", np.float32)
    assert fb_file.shape == ((1 + K) * n, 4)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)            # (the fixture's dt, as tests/test_full_multi_cli.py)
        out, cand, fb = ctx.match_ncc_full_fb(xy, off, 16, 7, K, shift=shift)
        assert ctx.last_path() == ("f32i_full" if dn16 else "u8_mfma_full")
    assert_bits_equal(rec_file[:, :8], out, "record")
    assert_bits_equal(fb_file.reshape(1 + K, n, 4), fb, "fb")
    if K:
        assert_bits_equal(fileio.read_gma(f"{b}/candidates_{t0}_{t1}.GMA", np.float32).reshape(K, n, 3), cand, "candidates")
    assert np.isfinite(fb[0, :, 3]).any()


def test_fb_0_writes_todays_files(tmp_path):
    _, _, _, t0, t1, a, p = _run(tmp_path, "a", ["16", "7", "1", "3"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, _, _, _, b, p = _run(tmp_path, "b", ["16", "7", "1", "3", "0", "0"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, _, _, _, c, p = _run(tmp_path, "c", ["16", "7", "1", "3", "0", "1"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == [f"candidates_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt"]
    for name in os.listdir(a):
        assert open(f"{a}/{name}", "rb").read() == open(f"{b}/{name}", "rb").read(), name
        assert open(f"{a}/{name}", "rb").read() == open(f"{c}/{name}", "rb").read(), name + " (fb=1 leaves the other files alone)"


def test_fb_on_a_pyramid_is_refused(tmp_path):
    _, _, _, _, _, a, p = _run(tmp_path, "a", ["16", "7", "2", "1", "0", "1"])
    assert p.returncode != 0 and "levels = 1" in p.stderr
    assert os.listdir(a) == []


def test_fb_1_on_a_filtered_pair(tmp_path):
    """filter=1 with fb=1: fb_<t0>_<t1>_f1.GMA is the entry's array on the filtered pair, and the other files are those of the run
    without fb (there the search goes through mimc3_match_ncc_full_planes)."""
    from mimc3_amd import api
    z, i0, i1, t0, t1, a, p = _run(tmp_path, "a", ["16", "7", "1", "3", "1"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, _, _, _, b, p = _run(tmp_path, "b", ["16", "7", "1", "3", "1", "1"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(b)) == sorted(os.listdir(a) + [f"fb_{t0}_{t1}_f1.GMA"])
    for name in os.listdir(a):
        assert open(f"{a}/{name}", "rb").read() == open(f"{b}/{name}", "rb").read(), name
    xy = z["xyuvav"]
    n = xy.shape[0]
    line = open(f"{b}/offsets_{t0}_{t1}_f1.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        ctx.filter_images(api.CLI_KERNELS[0])
        _, _, fb = ctx.match_ncc_full_fb(xy, off, 16, 7, 3, shift=shift)
    assert_bits_equal(fileio.read_gma(f"{b}/fb_{t0}_{t1}_f1.GMA", np.float32).reshape(4, n, 4), fb, "fb on the filtered pair")


def test_fb_1_with_peaks_1_and_16bit_leaves_the_other_files_alone(tmp_path):
    """Without fb these runs go through mimc3_match_ncc_full (8-bit, peaks=1) and mimc3_match_ncc_full_dn (16-bit); with fb=1 through the
    new entry's forward pass: the same bytes."""
    for sub, dn16, peaks in (("a", False, "1"), ("b", True, "3")):
        os.makedirs(tmp_path / sub)
        _, _, _, _, _, x, p = _run(tmp_path / sub, "x", ["16", "7", "1", peaks], dn16=dn16)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        _, _, _, _, _, y, p = _run(tmp_path / sub, "y", ["16", "7", "1", peaks, "0", "1"], dn16=dn16)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert len(os.listdir(y)) == len(os.listdir(x)) + 1
        for name in os.listdir(x):
            assert open(f"{x}/{name}", "rb").read() == open(f"{y}/{name}", "rb").read(), name
