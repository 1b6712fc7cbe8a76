"""GPU: the coarse-to-fine exhaustive search (mimc3_match_ncc_pyramid: the levels of the 8-bit pair, one exhaustive search per level on
the matrix cores, the chaining on the device) against its test-side definition (tests/pyramid_oracle.py): the record as
assert_records_match compares it (bit for bit but the SNR, within 1 f32 ulp) and shift_out exactly."""
import os
import re
import subprocess

import numpy as np
import pytest

import fileio
from conftest import ROOT, assert_bits_equal, golden_files
from full_search_common import assert_records_match
from mimc3_amd import synth
from pyramid_oracle import BIG, big_case, pyramid_search

pytestmark = pytest.mark.gpu

MX_OCW = (7, 15, 16, 30, 32, 40)
CLI = os.path.join(ROOT, "mimc3_amd", "csrc", "MIMC3_hip_offsets")


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def case(ocw, null_frac, seed, levels=3):
    """odd image sizes (the reductions drop a row and a column), a coarsest level that holds a chip, a motion the prior misses by a few px"""
    h = (2 * ocw + 1) * (1 << (levels - 1)) + 45
    return synth.make_small(seed=seed, shift=(9, -7), angle_deg=40.0, ocw=ocw, speed=700.0, h=h, w=h + 14, dimx=6, dimy=5,
                            noise_dn=2, null_frac=null_frac, offset=(1, -1), sigma=3.0)


def test_one_level_is_match_ncc_full(api):
    c = case(16, 0.03, 8101)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        rec, sh = ctx.match_ncc_pyramid(c.xyuvav, c.offset, 16, 9, 1, shift=shift)
        assert ctx.last_path() == "u8_mfma_full"
        want = ctx.match_ncc_full(c.xyuvav, c.offset, 16, 9, shift=shift)
        rec0, sh0 = ctx.match_ncc_pyramid(c.xyuvav, c.offset, 16, 9, 1)
        want0 = ctx.match_ncc_full(c.xyuvav, c.offset, 16, 9)
    np.testing.assert_array_equal(sh, shift)
    assert_bits_equal(rec, want, "L = 1")
    assert not sh0.any()
    assert_bits_equal(rec0, want0, "L = 1, no shift")


@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("null_frac", [0.0, 0.03, 0.15])
@pytest.mark.parametrize("ocw", MX_OCW)
def test_oracle_parity(api, ocw, null_frac, levels):
    """Every chip size, null fraction and level count, both directions; match_ncc_full at shift_out reproduces the record."""
    c = case(ocw, null_frac, 8200 + ocw + int(100 * null_frac) + levels, levels)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    R = 6
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for swap in (False, True):
            off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
            rec, sh = ctx.match_ncc_pyramid(c.xyuvav, off, ocw, R, levels, shift=sh_in, swap=swap)
            what = f"ocw {ocw} nulls {null_frac} L {levels} swap {swap}"
            want, want_sh = pyramid_search(c.i0, c.i1, c.xyuvav, off, ocw, R, levels, shift=sh_in, swap=swap)
            np.testing.assert_array_equal(sh, want_sh, what)
            assert_records_match(rec, want, what)
            assert_bits_equal(ctx.match_ncc_full(c.xyuvav, off, ocw, R, shift=sh, swap=swap), rec, what + " vs match_ncc_full")


def test_large_displacement(api):
    """(+70, -45) px with no prior: one level at R 15 finds it at under 10 % of the points, three levels at >= 90 % of the valid ones."""
    i0, i1, g = big_case()
    du, dv = BIG["motion"]
    ocw = BIG["ocw"]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        one = ctx.match_ncc_full(g, (0, 0), ocw, 15)
        rec, sh = ctx.match_ncc_pyramid(g, (0, 0), ocw, 15, 3)
    hit1 = (np.abs(one[:, 0] - du) < 0.05) & (np.abs(one[:, 1] - dv) < 0.05)
    assert hit1.mean() < 0.1
    ok = rec[:, 2] >= -1
    hit = ok & (np.abs(rec[:, 0] - du) < 0.05) & (np.abs(rec[:, 1] - dv) < 0.05)
    assert ok.sum() > 0 and hit.sum() >= 0.9 * ok.sum()
    want, want_sh = pyramid_search(i0, i1, g, (0, 0), ocw, 15, 3)
    np.testing.assert_array_equal(sh, want_sh)
    assert_records_match(rec, want, "(+70, -45)")


def test_boxes_beyond_the_zero_border(api):
    """Points whose derived level-0 search box leaves the 256-px zero border get the all-NaN record; the call is not refused."""
    c = case(15, 0.0, 8301)
    shift = np.zeros((c.n, 2), np.int32)
    shift[::3] = (400, 0)                              # coarser levels search zeros (-3: no arg-max); level 0's boxes leave the border
    shift[1::3] = (0, -280)                            # level 0's boxes leave the border on the top row of points only
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        rec, sh = ctx.match_ncc_pyramid(c.xyuvav, (0, 0), 15, 15, 3, shift=shift)
        ok = ctx.match_ncc_pyramid(c.xyuvav, (0, 0), 15, 15, 3)[0]        # the context still works
    want, want_sh = pyramid_search(c.i0, c.i1, c.xyuvav, (0, 0), 15, 15, 3, shift=shift)
    np.testing.assert_array_equal(sh, want_sh)
    assert_records_match(rec, want, "beyond the border")
    assert np.isnan(rec[::3]).all()
    assert np.isnan(rec).all(axis=1).sum() > len(rec[::3])
    assert (ok[:, 2] >= -1).any()


def test_pair_changes(api):
    """A pyramid on pair A, then set_images / set_images_raw (8-bit DN) to pair B: B's result is a fresh context's; a DLC pass gives the same
    bytes before and after a pyramid call."""
    a = case(16, 0.03, 8401)
    b = case(16, 0.03, 8402)
    shift = api.prior_shift(b.xyuvav, b.dt, b.mpp)
    H, W = b.i0.shape
    off, uv = api.get_uv_pivot(b.xyuvav, b.dt, b.mpp, 16, H, W)
    with api.Context(0) as fresh:
        fresh.set_images(b.i0, b.i1)
        want = fresh.match_ncc_pyramid(b.xyuvav, b.offset, 16, 7, 3, shift=shift)
    with api.Context(0) as ctx:
        ctx.set_images(a.i0, a.i1)
        ctx.match_ncc_pyramid(a.xyuvav, a.offset, 16, 7, 3)
        ctx.set_images(b.i0, b.i1)
        got = ctx.match_ncc_pyramid(b.xyuvav, b.offset, 16, 7, 3, shift=shift)
        dlc0 = ctx.matching_ncc_dlc_2(b.xyuvav, b.offset, off, uv, 16)
        ctx.match_ncc_pyramid(b.xyuvav, b.offset, 16, 7, 2, shift=shift)
        dlc1 = ctx.matching_ncc_dlc_2(b.xyuvav, b.offset, off, uv, 16)
        ctx.set_images_raw(a.i0.astype(np.uint8), a.i1.astype(np.uint8))     # (mimc3_ctx_set_images_u8)
        ctx.match_ncc_pyramid(a.xyuvav, a.offset, 16, 7, 3)
        ctx.set_images_raw(b.i0.astype(np.uint8), b.i1.astype(np.uint8))
        got_u8 = ctx.match_ncc_pyramid(b.xyuvav, b.offset, 16, 7, 3, shift=shift)
    for g, what in ((got, "set_images"), (got_u8, "set_images_u8")):
        assert_bits_equal(g[0], want[0], what)
        np.testing.assert_array_equal(g[1], want[1], what)
    assert_bits_equal(dlc1, dlc0, "DLC around a pyramid call")


def test_device_twin(api):
    from hipmem import DevArray
    c = case(30, 0.03, 8501)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        rec, sh = ctx.match_ncc_pyramid(c.xyuvav, c.offset, 30, 8, 3, shift=shift)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
        d_out, d_sho = DevArray((c.n, 8), np.float32), DevArray((c.n, 2), np.int32)
        ctx.match_ncc_pyramid_dev(d_xy.ptr, c.n, c.offset, 30, 8, 3, d_out.ptr, d_shift=d_sh.ptr, d_shift_out=d_sho.ptr)
        dev, dev_sh = d_out.numpy(), d_sho.numpy()
        d_out2 = DevArray((c.n, 8), np.float32)
        ctx.match_ncc_pyramid_dev(d_xy.ptr, c.n, c.offset, 30, 8, 3, d_out2.ptr, d_shift=d_sh.ptr)
        dev2 = d_out2.numpy()
    assert_bits_equal(dev, rec, "_dev twin")
    assert_bits_equal(dev2, rec, "_dev twin without shift_out")
    np.testing.assert_array_equal(dev_sh, sh)


def test_refusals(api):
    c = case(7, 0.0, 8601)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for ocw, radius, levels in ((7, 0, 2), (7, 16, 2), (8, 5, 2), (7, 5, 0), (7, 5, 6)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_pyramid(c.xyuvav, (0, 0), ocw, radius, levels)
            assert e.value.code == -1
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid(c.xyuvav, (1 << 25, 0), 7, 5, 2)
        assert e.value.code == -1
        xy = c.xyuvav.copy()
        xy[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid(xy, (0, 0), 7, 5, 2)
        assert e.value.code == -2
        ctx.set_images(c.i0 * 4, c.i1 * 4)                          # 10-bit values: the u16 planes
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid(c.xyuvav, (0, 0), 7, 5, 2)
        assert e.value.code == -6
    # a pair too small for the coarsest level's chip
    i0 = synth.texture(120, 130, 4)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i0)
        xy = np.zeros((1, 6))
        xy[0, 2:4] = (60, 60)
        ctx.match_ncc_pyramid(xy, (0, 0), 7, 5, 4)                # level 3 is 15 x 16: it holds a 15-px chip
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid(xy, (0, 0), 7, 5, 5)            # level 4 is 7 x 8: it does not
        assert e.value.code == -1


def test_full_size_c2_sample(api):
    """C2 (4096^2, 200,000 points, ocw 16, R 15, three levels): the whole pass on the device, a 20,000-point sample against the
    definition."""
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        rec, sh = ctx.match_ncc_pyramid(c.xyuvav, c.offset, 16, 15, 3, shift=shift)
    sel = np.random.default_rng(2).choice(c.n, 20000, replace=False)
    sel.sort()
    want, want_sh = pyramid_search(c.i0, c.i1, c.xyuvav[sel], c.offset, 16, 15, 3, shift=shift[sel])
    np.testing.assert_array_equal(sh[sel], want_sh)
    assert_records_match(rec[sel], want, "C2 sample")
    assert (rec[:, 2] >= -1).mean() > 0.9


def _run_cli(tmp_path, z, args):
    t0, t1 = str(z["t0"]), str(z["t1"])
    d = str(tmp_path)
    os.makedirs(f"{d}/out")
    fileio.write_tiff(f"{d}/{t0}_i0.tif", z["i0"].astype(np.uint8))
    fileio.write_tiff(f"{d}/{t1}_i1.tif", z["i1"].astype(np.uint8))
    fileio.write_gma(f"{d}/xyuvav.GMA", z["xyuvav"])
    p = subprocess.run([CLI, f"{d}/{t0}_i0.tif", f"{d}/{t1}_i1.tif", f"{d}/xyuvav.GMA", f"{d}/out"] + args,
                       env=dict(os.environ, MIMC3_CP_SEED=str(int(z["seed"]))), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    base = f"{d}/out/offsets_{t0}_{t1}"
    return open(base + ".GMA", "rb").read(), open(base + ".txt").read()


def test_cli_levels(api, tmp_path):
    """levels > 1: the .GMA holds the Python entry's pyramid record for the same offset and a-priori shifts; levels=1 writes the files
    the command line writes without the argument, byte for byte."""
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mimc3_amd", "csrc"), "cli"])
    z = np.load(golden_files("vmap_small")[0])
    xy = z["xyuvav"]
    gma_default, txt_default = _run_cli(tmp_path / "a", z, ["15", "7"])
    gma_one, txt_one = _run_cli(tmp_path / "b", z, ["15", "7", "1"])
    assert gma_one == gma_default and txt_one == txt_default
    H = z["i0"].shape[0]
    levels = 2 if (H >> 2) < 31 else 3
    gma, txt = _run_cli(tmp_path / "c", z, ["15", "7", str(levels)])
    off = [int(v) for v in re.search(r"control-point offset (-?\d+) (-?\d+)", txt).groups()]
    out = tmp_path / "c" / "out"
    got = fileio.read_gma(str(out / [f for f in os.listdir(out) if f.endswith(".GMA")][0]), np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(z["i0"].astype(np.float32), z["i1"].astype(np.float32))
        shift = api.prior_shift(xy, 16.0, ctx.vmap_geometry(xy).mpp)
        want, _ = ctx.match_ncc_pyramid(xy, off, 15, 7, levels, shift=shift)
    assert got.shape == (xy.shape[0], 10)
    assert_bits_equal(got[:, :8], want, "CLI pyramid record")
    rows = [ln for ln in txt.splitlines()[1:] if ln.strip()]
    assert len(rows) == int((want[:, 2] >= -1).sum())
