"""GPU: the filter argument of the MIMC3_hip_offsets command line: filter=0 writes byte-identical files to a run without the argument;
filter=1 peaks=3 writes offsets_<t0>_<t1>_f1.GMA / .txt and candidates_<t0>_<t1>_f1.GMA, equal to the API path (filter_images, then
match_ncc_full_planes) for the offset the run reports; filter=1 with levels=2 is refused and nothing is written."""
import os
import re

import numpy as np
import pytest

import fileio
from conftest import assert_bits_equal
from test_full_multi_cli import _run

pytestmark = pytest.mark.gpu


def test_filter_0_writes_todays_files(tmp_path):
    _, t0, t1, a, p = _run(tmp_path, "a", ["16", "7", "1", "3"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, _, b, p = _run(tmp_path, "b", ["16", "7", "1", "3", "0"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == [f"candidates_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.GMA", f"offsets_{t0}_{t1}.txt"]
    for name in os.listdir(a):
        assert open(f"{a}/{name}", "rb").read() == open(f"{b}/{name}", "rb").read(), name


def test_filter_1_equals_the_api_path(tmp_path):
    from mimc3_amd import api
    z, t0, t1, b, p = _run(tmp_path, "b", ["16", "7", "1", "3", "1"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(b)) == [f"candidates_{t0}_{t1}_f1.GMA", f"offsets_{t0}_{t1}_f1.GMA", f"offsets_{t0}_{t1}_f1.txt"]
    xy = z["xyuvav"]
    n = xy.shape[0]
    line = open(f"{b}/offsets_{t0}_{t1}_f1.txt").readline()
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", line).groups()]
    rec_file = fileio.read_gma(f"{b}/offsets_{t0}_{t1}_f1.GMA", np.float32)
    cand_file = fileio.read_gma(f"{b}/candidates_{t0}_{t1}_f1.GMA", np.float32)
    assert rec_file.shape == (n, 10) and cand_file.shape == (3 * n, 3)
    with api.Context(0) as ctx:
        ctx.set_images(z["i0"].astype(np.float32), z["i1"].astype(np.float32))
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)            # (the fixture's dt, as tests/test_full_multi_cli.py)
        ctx.filter_images(api.CLI_KERNELS[0])
        out, cand = ctx.match_ncc_full_planes(xy, off, 16, 7, 3, shift=shift)
    assert_bits_equal(rec_file[:, :8], out, "record")
    assert_bits_equal(cand_file.reshape(3, n, 3), cand, "candidates")
    assert (out[:, 2] >= -1).mean() > 0.5


def test_filter_with_levels_is_refused(tmp_path):
    _, _, _, b, p = _run(tmp_path, "b", ["16", "7", "2", "1", "1"])
    assert p.returncode != 0 and "filter" in p.stderr
    assert os.listdir(b) == []
