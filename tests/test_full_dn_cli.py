"""GPU: 16-bit TIFFs through the MIMC3_hip_offsets command line: the records and candidates it writes equal match_ncc_full_dn for the
offset the run reports, raw and with filter=1; levels=2 on a 16-bit pair is refused and nothing is written; one 8-bit and one 16-bit
file stay refused."""
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


def _run16(tmp_path, sub, args, mixed=False):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mimc3_amd", "csrc"), "cli"])
    z = np.load(golden_files("vmap_small")[0])
    t0, t1 = str(z["t0"]), str(z["t1"])
    d = str(tmp_path)
    i0, i1 = to_dn16(z["i0"], 11), to_dn16(z["i1"], 12)
    if not os.path.exists(f"{d}/xyuvav.GMA"):
        fileio.write_tiff(f"{d}/{t0}_i0.tif", i0.astype(np.uint16))
        fileio.write_tiff(f"{d}/{t1}_i1.tif", z["i1"].astype(np.uint8) if mixed else i1.astype(np.uint16))
        fileio.write_gma(f"{d}/xyuvav.GMA", z["xyuvav"])
    os.makedirs(f"{d}/{sub}")
    p = subprocess.run([CLI, f"{d}/{t0}_i0.tif", f"{d}/{t1}_i1.tif", f"{d}/xyuvav.GMA", f"{d}/{sub}"] + args,
                       env=dict(os.environ, MIMC3_CP_SEED=str(int(z["seed"]))), capture_output=True, text=True, timeout=300)
    return z, i0, i1, t0, t1, f"{d}/{sub}", p


@pytest.mark.parametrize("filt", [0, 1])
def test_16bit_run_equals_the_api_path(tmp_path, filt):
    from mimc3_amd import api
    z, i0, i1, t0, t1, b, p = _run16(tmp_path, "b", ["16", "7", "1", "3", str(filt)])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    sfx = f"_f{filt}" if filt else ""
    assert sorted(os.listdir(b)) == [f"candidates_{t0}_{t1}{sfx}.GMA", f"offsets_{t0}_{t1}{sfx}.GMA", f"offsets_{t0}_{t1}{sfx}.txt"]
    xy = z["xyuvav"]
    n = xy.shape[0]
    line = open(f"{b}/offsets_{t0}_{t1}{sfx}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    rec_file = fileio.read_gma(f"{b}/offsets_{t0}_{t1}{sfx}.GMA", np.float32)
    cand_file = fileio.read_gma(f"{b}/candidates_{t0}_{t1}{sfx}.GMA", np.float32)
    assert rec_file.shape == (n, 10) and cand_file.shape == (3 * n, 3)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)            # (the fixture's dt, as tests/test_full_multi_cli.py)
        if filt:
            ctx.filter_images(api.CLI_KERNELS[filt - 1])
        out, cand = ctx.match_ncc_full_dn(xy, off, 16, 7, 3, shift=shift)
        assert ctx.last_path() == "f32i_full"
    assert_bits_equal(rec_file[:, :8], out, "record")
    assert_bits_equal(cand_file.reshape(3, n, 3), cand, "candidates")
    assert (out[:, 2] >= -1).mean() > 0.5


def test_peaks_1_writes_the_record_alone(tmp_path):
    from mimc3_amd import api
    z, i0, i1, t0, t1, b, p = _run16(tmp_path, "b", ["16", "7"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(b)) == [f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt"]
    xy = z["xyuvav"]
    line = open(f"{b}/offsets_{t0}_{t1}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    rec_file = fileio.read_gma(f"{b}/offsets_{t0}_{t1}.GMA", np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        out, _ = ctx.match_ncc_full_dn(xy, off, 16, 7, 0, shift=shift)
    assert_bits_equal(rec_file[:, :8], out, "record")


def test_levels_on_a_16bit_pair_are_refused(tmp_path):
    _, _, _, _, _, b, p = _run16(tmp_path, "b", ["16", "7", "2"])
    assert p.returncode != 0 and "levels = 1" in p.stderr
    assert os.listdir(b) == []


def test_mixed_depths_stay_refused(tmp_path):
    _, _, _, _, _, b, p = _run16(tmp_path, "b", ["16", "7"], mixed=True)
    assert p.returncode != 0 and "8-bit or two 16-bit" in p.stderr
    assert os.listdir(b) == []
