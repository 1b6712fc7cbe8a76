"""GPU: chip half-widths other than the six on the MIMC3_hip_offsets command line.  `... 10 7 1 4` on an 8-bit pair and `... 10 7 1 1 1`
(filter 1) on a 16-bit pair write offsets_* and candidates_* files that hold exactly what Context.match_ncc_full_chip (mode 0) returns
for the same points, offset and shift; ocw 16 keeps writing what the entries it has always called return; levels > 1, fb = 1 and R > 15
with such an ocw, and an ocw outside 1..80, are refused with the limit named and nothing written."""
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


def _files(b, t0, t1, tag, K):
    line = open(f"{b}/offsets_{t0}_{t1}{tag}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    rec = fileio.read_gma(f"{b}/offsets_{t0}_{t1}{tag}.GMA", np.float32)
    cand = fileio.read_gma(f"{b}/candidates_{t0}_{t1}{tag}.GMA", np.float32) if K else None
    return off, rec, cand


@pytest.mark.parametrize("dn16,filt,K", [(False, 0, 4), (True, 1, 0)], ids=["8bit_peaks4", "16bit_filter1"])
def test_ocw10_writes_the_library_calls_arrays(tmp_path, dn16, filt, K):
    from mimc3_amd import api
    ocw, R = 10, 7
    z, i0, i1, t0, t1, b, p = _run(tmp_path, "b", [str(ocw), str(R), "1", str(K or 1), str(filt)], dn16=dn16)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    tag = f"_f{filt}" if filt else ""
    names = [f"offsets_{t0}_{t1}{tag}.GMA", f"offsets_{t0}_{t1}{tag}.txt"] + ([f"candidates_{t0}_{t1}{tag}.GMA"] if K else [])
    assert sorted(os.listdir(b)) == sorted(names)
    xy = z["xyuvav"]
    n = xy.shape[0]
    off, rec_file, cand_file = _files(b, t0, t1, tag, K)
    assert rec_file.shape == (n, 10)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)            # (the fixture's dt, as tests/test_wide_cli.py)
        if filt:
            ctx.filter_images(api.CLI_KERNELS[filt - 1])
        out, cand = ctx.match_ncc_full_chip(xy, off, ocw, R, K, shift=shift)
        assert ctx.last_path() == "f32g_chip"
    assert_bits_equal(rec_file[:, :8], out, "record vs match_ncc_full_chip")
    if K:
        assert cand_file.shape == (K * n, 3)
        assert_bits_equal(cand_file.reshape(K, n, 3), cand, "candidates vs match_ncc_full_chip")
    assert np.array_equal(rec_file[:, 8:], xy[:, 2:4].astype(np.float32))
    assert np.isfinite(out[:, 0]).sum() >= n // 4


def test_ocw16_keeps_its_calls(tmp_path):
    from mimc3_amd import api
    ocw, R, K = 16, 7, 3
    z, i0, i1, t0, t1, b, p = _run(tmp_path, "b", [str(ocw), str(R), "1", str(K)])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    xy = z["xyuvav"]
    n = xy.shape[0]
    off, rec_file, cand_file = _files(b, t0, t1, "", K)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        out, cand = ctx.match_ncc_full_multi(xy, off, ocw, R, K, shift=shift)
        assert ctx.last_path() == "u8_mfma_full"
    assert_bits_equal(rec_file[:, :8], out, "record vs match_ncc_full_multi")
    assert_bits_equal(cand_file.reshape(K, n, 3), cand, "candidates vs match_ncc_full_multi")
    _, _, _, _, _, a, p = _run(tmp_path, "a", [str(ocw), str(R)])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        assert_bits_equal(fileio.read_gma(f"{a}/offsets_{t0}_{t1}.GMA", np.float32)[:, :8], ctx.match_ncc_full(xy, off, ocw, R, shift=shift),
                          "record vs match_ncc_full")


@pytest.mark.parametrize("args,words", [(["10", "7", "2"], ("levels = 1",)), (["10", "7", "1", "1", "0", "1"], ("fb = 0",)),
                                        (["10", "16"], ("R <= 15",)), (["81", "7"], ("1..80",)), (["0", "7"], ("1..80",))],
                         ids=["levels2", "fb1", "R16", "ocw81", "ocw0"])
def test_refusals_write_nothing(tmp_path, args, words):
    _, _, _, _, _, a, p = _run(tmp_path, "a", args)
    assert p.returncode != 0 and all(w in p.stderr for w in words), p.stderr[-2000:]
    assert os.listdir(a) == []
