"""GPU: MIMC3_hip_offsets at a chip half-width other than the six on 8-bit TIFFs goes through mimc3_match_ncc_full_chip_class: `... 10 7 1 4`
writes offsets_* and candidates_* files that hold exactly what Context.match_ncc_full_chip_class (mode 0) returns for the same points,
offset and shift -- the matrix-core kernel's result ("u8_mfma_chip"), which is also match_ncc_full_chip's bytes."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from test_full_chip_cli import _files, _run

pytestmark = pytest.mark.gpu


def test_ocw10_peaks4_writes_the_new_library_calls_bytes(tmp_path):
    from mimc3_amd import api
    ocw, R, K = 10, 7, 4
    z, i0, i1, t0, t1, b, p = _run(tmp_path, "b", [str(ocw), str(R), "1", str(K)])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    xy = z["xyuvav"]
    n = xy.shape[0]
    off, rec_file, cand_file = _files(b, t0, t1, "", K)
    assert rec_file.shape == (n, 10) and cand_file.shape == (K * n, 3)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        out, cand = ctx.match_ncc_full_chip_class(xy, off, ocw, R, K, shift=shift)
        assert ctx.last_path() == "u8_mfma_chip"
        old = ctx.match_ncc_full_chip(xy, off, ocw, R, K, shift=shift, mode=1)
    assert_bits_equal(rec_file[:, :8], out, "record vs match_ncc_full_chip_class")
    assert_bits_equal(cand_file.reshape(K, n, 3), cand, "candidates vs match_ncc_full_chip_class")
    assert_bits_equal(out, old[0], "record vs match_ncc_full_chip(mode 1)")
    assert_bits_equal(cand, old[1], "candidates vs match_ncc_full_chip(mode 1)")
    assert np.isfinite(out[:, 0]).sum() >= n // 4
