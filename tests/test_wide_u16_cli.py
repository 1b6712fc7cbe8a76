"""GPU: R beyond 15 on the MIMC3_hip_offsets command line on a FILTERED pair goes through mimc3_match_ncc_wide_planes in mode 0: at ocw 16,
R 20, filter 1 (d/dx) and 3 (Laplacian), peaks 1 and 4, the files hold exactly what Context.match_ncc_wide returns on the filtered pair for
the same points, the offset the run reports and the a-priori shift -- and the library entry the command line calls runs a matrix-core
kernel there: the u8-plane one on the d/dx pair, which is still an 8-bit pair, the u16-plane one on the Laplacian pair (and on both in mode 1)."""
import os
import re
import subprocess

import numpy as np
import pytest

import fileio
from conftest import ROOT, assert_bits_equal, golden_files

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mimc3_amd", "csrc", "MIMC3_hip_offsets")


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("filt", [1, 3])
def test_r20_on_a_filtered_pair_writes_match_ncc_wides_arrays(tmp_path, filt, K):
    from mimc3_amd import api
    assert hasattr(api.Context, "match_ncc_wide_planes")            # (the entry the command line calls)
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mimc3_amd", "csrc"), "cli"])
    ocw, R = 16, 20
    z = np.load(golden_files("vmap_small")[0])
    t0, t1, d = str(z["t0"]), str(z["t1"]), str(tmp_path)
    i0, i1, xy = z["i0"].astype(np.float32), z["i1"].astype(np.float32), z["xyuvav"]
    n = xy.shape[0]
    fileio.write_tiff(f"{d}/{t0}_i0.tif", i0.astype(np.uint8))
    fileio.write_tiff(f"{d}/{t1}_i1.tif", i1.astype(np.uint8))
    fileio.write_gma(f"{d}/xyuvav.GMA", xy)
    os.makedirs(f"{d}/out")
    p = subprocess.run([CLI, f"{d}/{t0}_i0.tif", f"{d}/{t1}_i1.tif", f"{d}/xyuvav.GMA", f"{d}/out", str(ocw), str(R), "1", str(K), str(filt)],
                       env=dict(os.environ, MIMC3_CP_SEED=str(int(z["seed"]))), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    tag = f"_f{filt}"
    names = [f"offsets_{t0}_{t1}{tag}.GMA", f"offsets_{t0}_{t1}{tag}.txt"] + ([f"candidates_{t0}_{t1}{tag}.GMA"] if K > 1 else [])
    assert sorted(os.listdir(f"{d}/out")) == sorted(names)
    line = open(f"{d}/out/offsets_{t0}_{t1}{tag}.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    rec_file = fileio.read_gma(f"{d}/out/offsets_{t0}_{t1}{tag}.GMA", np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        ctx.filter_images(api.CLI_KERNELS[filt - 1])
        w_out, w_cand = ctx.match_ncc_wide(xy, off, ocw, R, K if K > 1 else 0, shift=shift)
        assert ctx.last_path() == "f32g_wide"
        # mode 0, the command line's call: a filtered pair that is still 8-bit (integers 0..255: the d/dx pair here) goes where
        # match_ncc_wide_class sends an 8-bit pair, a scaled-integer one (the Laplacian's eighths) to the u16-plane kernel
        f0, f1 = ctx.get_images(*i0.shape)
        is8 = all(np.array_equal(f, np.rint(f)) and f.min() >= 0 and f.max() <= 255 for f in (f0, f1))
        assert is8 == (filt == 1)
        c_out, c_cand = ctx.match_ncc_wide_planes(xy, off, ocw, R, K if K > 1 else 0, shift=shift)
        assert ctx.last_path() == ("u8_mfma_wide" if is8 else "u16_mfma_wide")
        m_out, m_cand = ctx.match_ncc_wide_planes(xy, off, ocw, R, K if K > 1 else 0, shift=shift, mode=1)      # the u16-plane kernel on both
        assert ctx.last_path() == "u16_mfma_wide"
    assert_bits_equal(m_out, w_out, "match_ncc_wide_planes(mode 1) vs match_ncc_wide")
    if K > 1:
        assert_bits_equal(m_cand, w_cand, "match_ncc_wide_planes(mode 1) candidates vs match_ncc_wide")
    assert rec_file.shape == (n, 10)
    assert_bits_equal(rec_file[:, :8], w_out, "record vs match_ncc_wide")
    assert_bits_equal(c_out, w_out, "match_ncc_wide_planes vs match_ncc_wide")
    if K > 1:
        cand_file = fileio.read_gma(f"{d}/out/candidates_{t0}_{t1}{tag}.GMA", np.float32)
        assert_bits_equal(cand_file.reshape(K, n, 3), w_cand, "candidates vs match_ncc_wide")
        assert_bits_equal(c_cand, w_cand, "match_ncc_wide_planes candidates vs match_ncc_wide")
    assert np.array_equal(rec_file[:, 8:], xy[:, 2:4].astype(np.float32)) and np.isfinite(w_out[:, 0]).sum() >= n // 4
