"""GPU: MIMC3_hip_offsets at a chip half-width other than the six with a filter on 8-bit TIFFs goes through
mimc3_match_ncc_full_chip_planes: `... 10 7 1 4 <filter>` writes offsets_*_f<k> and candidates_*_f<k> files whose arrays are exactly what
match_ncc_full_chip returns after filter_images(kernel k) for the same points, offset and shift.  The class of the fixture's filtered pair
is known: its d/dx pair (filter 1) has integers 0..247 and classes as 8-bit, so the program's mode-0 call runs "u8_mfma_chip"; its
Laplacian pair (filter 3) holds eighths and runs the matrix-core kernel on the u16 planes, "u16_mfma_chip".  Mode 1 forces that kernel
on both: the same bytes."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from test_full_chip_cli import _files, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("filt,path", [(1, "u8_mfma_chip"), (3, "u16_mfma_chip")], ids=["ddx", "laplacian"])
def test_ocw10_filter_peaks4_writes_the_library_calls_bytes(tmp_path, filt, path):
    from mimc3_amd import api
    ocw, R, K = 10, 7, 4
    z, i0, i1, t0, t1, b, p = _run(tmp_path, "b", [str(ocw), str(R), "1", str(K), str(filt)])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    xy = z["xyuvav"]
    n = xy.shape[0]
    off, rec_file, cand_file = _files(b, t0, t1, f"_f{filt}", K)
    assert rec_file.shape == (n, 10) and cand_file.shape == (K * n, 3)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        ctx.filter_images(api.CLI_KERNELS[filt - 1])
        out, cand = ctx.match_ncc_full_chip_planes(xy, off, ocw, R, K, shift=shift)        # the program's call
        assert ctx.last_path() == path
        forced = ctx.match_ncc_full_chip_planes(xy, off, ocw, R, K, shift=shift, mode=1)
        assert ctx.last_path() == "u16_mfma_chip"
        old = ctx.match_ncc_full_chip(xy, off, ocw, R, K, shift=shift, mode=1)
        assert ctx.last_path() == "f32g_chip"
    assert_bits_equal(rec_file[:, :8], old[0], "record vs match_ncc_full_chip after filter_images")
    assert_bits_equal(cand_file.reshape(K, n, 3), old[1], "candidates vs match_ncc_full_chip after filter_images")
    assert_bits_equal(out, old[0], "match_ncc_full_chip_planes: record")
    assert_bits_equal(cand, old[1], "match_ncc_full_chip_planes: candidates")
    assert_bits_equal(forced[0], old[0], "match_ncc_full_chip_planes(mode 1): record")
    assert_bits_equal(forced[1], old[1], "match_ncc_full_chip_planes(mode 1): candidates")
    assert np.isfinite(out[:, 0]).sum() >= n // 4
