"""GPU: null pixels that are not +0.0 and points at the 80 % invalid-pixel limit, through the C ABI, against the port oracle
(which tests/test_null_encodings_oracle.py pins to the compiled reference on the same inputs).

Integral valid DN with nulls in any encoding give bit-identical out[N,3]: a null never enters a sum, so every f64 sum stays an exact
integer in any order.  The kernels each restate the reference's rule (null for the sums: !(x >= THR), NaN included; invalid for the
80 % test: x < THR, NaN not counted) in their own form -- byte masks, null counts in the summed-area tables, bad/excluded counters,
closed-form T4 counts -- and the classifier must send every pair that is not 8-bit / scaled-integer to the f32 kernels."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import null_encoding_common as nc
from conftest import ROOT, assert_bits_equal
from full_search_common import assert_records_match, full_search

pytestmark = pytest.mark.gpu

OCW = (7, 15, 16, 30, 32, 40)
MODES = ("auto", "u8px", "u16", "f32", "general")
F32_MODES = ("auto", "f32", "general")
U8_PATH = {"auto": "u8_mfma", "u8px": "u8_exact", "u16": "u16_scaled", "f32": "f32_tiled", "general": "general_f32"}


def expected_path(mode, u8):
    """-0.0 passes "v >= 0 and integral" and keeps the pair 8-bit; NaN, negatives and 1e-11 leave the u8, u16 and integer-f32
    planes: the register-tiled f32 kernel, or the general one when forced."""
    return U8_PATH[mode] if u8 else ("general_f32" if mode == "general" else "f32_tiled")


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def oracle_pair(api, oracle, c):
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, c.ocw, H, W)
    return off, uv, (oracle.match(c.i0, c.i1, c.xyuvav, c.offset, off, uv, c.ocw),
                     oracle.match(c.i1, c.i0, c.xyuvav, -c.offset, off, -uv, c.ocw))


def run_modes(api, c, off, uv, modes, u8):
    """{mode: (forward, swapped)} on one context; asserts the path each mode takes."""
    res = {}
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for mode in modes:
            ctx.set_path(mode)
            fw = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, c.ocw)
            assert ctx.last_path() == expected_path(mode, u8), mode
            sw = ctx.matching_ncc_dlc_2(c.xyuvav, -c.offset, off, -uv, c.ocw, swap=True)
            assert ctx.last_path() == expected_path(mode, u8), mode + " swapped"
            res[mode] = (fw, sw)
    return res


# ---- (a) null encodings on every path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocw", OCW)
@pytest.mark.parametrize("enc", list(nc.ENCODINGS))
def test_null_encodings(api, oracle, enc, ocw):
    c = nc.encoded_case(ocw, enc)
    off, uv, (want, want_sw) = oracle_pair(api, oracle, c)
    assert (want[:, 2] > 0.5).sum() > len(want) // 2
    for mode, (fw, sw) in run_modes(api, c, off, uv, MODES, enc in nc.U8_ENCODINGS).items():
        assert_bits_equal(fw, want, f"{enc} ocw {ocw} {mode}")
        assert_bits_equal(sw, want_sw, f"{enc} ocw {ocw} {mode} swapped")


@pytest.mark.parametrize("enc", ["nan", "minus1"])
def test_single_null_in_the_last_pixel(api, oracle, enc):
    """8-bit everywhere but the last pixel of image 1: the classifiers' tails must see it (f32 kernels, not u8 / u16)."""
    c = nc.last_pixel_case(enc)
    off, uv, (want, want_sw) = oracle_pair(api, oracle, c)
    for mode, (fw, sw) in run_modes(api, c, off, uv, MODES, False).items():
        assert_bits_equal(fw, want, f"{enc} {mode}"); assert_bits_equal(sw, want_sw, f"{enc} {mode} swapped")


@pytest.mark.parametrize("ocw", OCW)
def test_threshold_valued_pixels(api, oracle, ocw):
    """Valid pixels equal to THR (~1.0000000133e-10, the smallest valid f32) at 5 % of each image: the sums are no longer exact, so
    the file's float tolerance applies (<= 1e-4 px, NCC <= 1e-6, the same invalid mask).  A kernel that took THR for a null would
    break it: test_null_encodings_oracle.py::test_threshold_pixels_are_not_nulls shows that the oracle's output then moves by more
    than 1e-3 px or 1e-4 in NCC (or changes its NaN mask) at every chip size."""
    c = nc.threshold_case(ocw)
    off, uv, want = oracle_pair(api, oracle, c)
    for mode, got in run_modes(api, c, off, uv, MODES, False).items():
        for g, w, what in zip(got, want, ("forward", "swapped")):
            assert np.array_equal(np.isnan(g), np.isnan(w)), f"ocw {ocw} {mode} {what}: NaN masks"
            assert np.array_equal(g[:, 2] == -3, w[:, 2] == -3), f"ocw {ocw} {mode} {what}: invalid masks"
            assert np.nanmax(np.abs(g[:, :2] - w[:, :2])) <= 1e-4, f"ocw {ocw} {mode} {what}: du, dv"
            assert np.nanmax(np.abs(g[:, 2] - w[:, 2])) <= 1e-6, f"ocw {ocw} {mode} {what}: NCC"


@pytest.mark.parametrize("ocw", OCW)
def test_positive_infinity(api, oracle, ocw):
    """+inf is a valid pixel: the sums of the cells that reach it turn inf - inf = NaN in any order."""
    c = nc.inf_case(ocw)
    off, uv, (want, want_sw) = oracle_pair(api, oracle, c)
    assert np.isnan(want[:, 0]).any()
    for mode, (fw, sw) in run_modes(api, c, off, uv, MODES, False).items():
        assert_bits_equal(fw, want, f"ocw {ocw} {mode}"); assert_bits_equal(sw, want_sw, f"ocw {ocw} {mode} swapped")


# ---- (b) the 80 % limit --------------------------------------------------------------------------------------------------------------
def limit_want(oracle, c):
    return oracle.match(c.chip_img, c.win_img, c.xyuvav, c.offset, c.piv_off, c.piv_uv, c.ocw)


@pytest.mark.parametrize("enc", ["zero", "minus1", "nan"])
@pytest.mark.parametrize("ocw", OCW)
def test_invalid_limit(api, oracle, ocw, enc):
    """k - 1, k, k + 1 invalid pixels in the chip and in the search area (T4 included; written nulls off and on the last written row
    and column), and a chip / a search area null throughout: -3 exactly from k on.  NaN nulls are not counted: every point stays
    valid, the all-NaN ones included.  Both directions (the swapped pass takes its chips from image 1)."""
    c = nc.limit_case(ocw, enc, lambda xy, o, H, W: oracle.get_uv_pivot(xy, 16.0, 15.0, o, H, W))
    want = limit_want(oracle, c)
    assert np.array_equal(want[:, 2] == -3, c.expect_invalid(enc not in nc.NOT_COUNTED))
    u8 = enc in nc.U8_ENCODINGS
    with api.Context(0) as ctx:
        for mode in (MODES if u8 else F32_MODES):
            ctx.set_path(mode)
            ctx.set_images(c.chip_img, c.win_img)
            got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw)
            assert ctx.last_path() == expected_path(mode, u8)
            assert_bits_equal(got, want, f"ocw {ocw} {enc} {mode}")
            ctx.set_images(c.win_img, c.chip_img)
            got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw, swap=True)
            assert_bits_equal(got, want, f"ocw {ocw} {enc} {mode} swapped")


def test_invalid_limit_on_the_matrix_core_null_forms():
    """The same 8-bit points with the matrix-core kernel's window-null and general forms switched on (they are off by default: the
    register-tiled kernel takes null-ridden points), where the search area's count is the table's written nulls + the closed-form
    T4 term Dx2 + Dy2 - 1.  A subprocess: the switches are read once per process."""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
        import null_encoding_common as nc
        from conftest import assert_bits_equal
        from mimc3_amd import api
        from oracle import oracle as orc
        o = orc.Oracle("port")
        for ocw in (7, 15, 16, 30, 32, 40):
            c = nc.limit_case(ocw, "zero", lambda xy, q, H, W: o.get_uv_pivot(xy, 16.0, 15.0, q, H, W))
            want = o.match(c.chip_img, c.win_img, c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw)
            with api.Context(0) as ctx:
                ctx.set_images(c.chip_img, c.win_img)
                got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw)
                assert ctx.last_path() == "u8_mfma"
                assert_bits_equal(got, want, "ocw %%d" %% ocw)
                ctx.set_images(c.win_img, c.chip_img)
                got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw, swap=True)
                assert_bits_equal(got, want, "ocw %%d swapped" %% ocw)
    """ % (ROOT, ROOT))
    env = dict(os.environ, MIMC3_MX_GEN="1", MIMC3_MX_WN="1")
    subprocess.check_call([sys.executable, "-c", code], env=env, timeout=300)


# ---- (c) pre-filter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(nc.CP_KERNELS)), ids=["ddx", "ddy", "laplacian"])
def test_prefilter_null_test_edges(api, oracle, k):
    """filter_images on pairs holding -1.5, nextafter(-1.5, 0), nextafter(0.5, 0), 0.5, NaN, -9999 and 3e9: the filtered planes
    bit for bit; then one matcher pass on the filtered pair (without 3e9, whose square is beyond exact f64 sums)."""
    kern = nc.CP_KERNELS[k]
    c = nc.conv2_case(huge=True)
    H, W = c.i0.shape
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        ctx.filter_images(kern)
        g0, g1 = ctx.get_images(H, W)
        assert_bits_equal(g0, oracle.float_conv2(c.i0, kern), "i0"); assert_bits_equal(g1, oracle.float_conv2(c.i1, kern), "i1")
        c = nc.conv2_case(huge=False)
        f0, f1 = oracle.float_conv2(c.i0, kern), oracle.float_conv2(c.i1, kern)
        off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, c.ocw, H, W)
        ctx.set_images(c.i0, c.i1)
        ctx.filter_images(kern)
        g0, g1 = ctx.get_images(H, W)
        assert_bits_equal(g0, f0, "i0 (no 3e9)"); assert_bits_equal(g1, f1, "i1 (no 3e9)")
        got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, c.ocw)
        want = oracle.match(f0, f1, c.xyuvav, c.offset, off, uv, c.ocw)
    assert_bits_equal(got, want, "matcher on the filtered pair")
    assert (want[:, 2] > 0).sum() > len(want) // 2


# ---- (d) control-point offset --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 99])
@pytest.mark.parametrize("enc", ["nan", "m9999"])
def test_cp_offset(api, oracle, enc, seed):
    i0, i1, xy = nc.cp_case(enc)
    rc, off, flag, info, sduv = oracle.get_offset_image(i0, i1, xy, nc.CP_KERNELS, seed, num_cp_min=20)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        st, o2, f2, info2, sduv2 = ctx.get_offset_image(xy, nc.CP_KERNELS, seed=seed, num_cp_min=20)
    assert st == rc
    assert np.array_equal(info2, info), (info2, info)
    assert np.array_equal(f2, flag)
    assert np.array_equal(sduv2.view(np.uint32), sduv.view(np.uint32)), (sduv2, sduv)
    assert np.array_equal(o2, off)


# ---- (e) exhaustive search -----------------------------------------------------------------------------------------------------------
MIMC3_EUNSUPPORTED = -6


def test_full_search_refuses_nan_nulls(api):
    c = nc.encoded_case(16, "nan")
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full(c.xyuvav, c.offset, 16, 7)
    assert e.value.code == MIMC3_EUNSUPPORTED


def test_full_search_negative_zero_nulls(api):
    """-0.0 nulls: the records of the same pair with +0.0 nulls, exactly."""
    recs = []
    for enc in ("zero", "negzero"):
        c = nc.encoded_case(16, enc)
        with api.Context(0) as ctx:
            ctx.set_images(c.i0, c.i1)
            recs.append((ctx.match_ncc_full(c.xyuvav, c.offset, 16, 7), ctx.match_ncc_full(c.xyuvav, -c.offset, 16, 7, swap=True)))
            assert ctx.last_path() == "u8_mfma_full"
    assert_bits_equal(recs[1][0], recs[0][0], "forward"); assert_bits_equal(recs[1][1], recs[0][1], "swapped")
    assert (recs[0][0][:, 2] == -3).sum() < len(recs[0][0]) // 2


def test_full_search_invalid_limit(api):
    """R 7, ocw 16: k - 1, k, k + 1 nulls in the chip and in the (2 (R + ocw) + 1)^2 search box (all of it read: no T4 term)."""
    c = nc.limit_case(16, "zero", radius=7)
    want = full_search(c.chip_img, c.win_img, c.xyuvav, c.offset, 16, 7)
    assert np.array_equal(want[:, 2] == -3, c.expect_invalid())
    want_sw = full_search(c.win_img, c.chip_img, c.xyuvav, c.offset, 16, 7, swap=True)
    with api.Context(0) as ctx:
        ctx.set_images(c.chip_img, c.win_img)
        assert_records_match(ctx.match_ncc_full(c.xyuvav, c.offset, 16, 7), want, "forward")
        assert ctx.last_path() == "u8_mfma_full"
        ctx.set_images(c.win_img, c.chip_img)
        assert_records_match(ctx.match_ncc_full(c.xyuvav, c.offset, 16, 7, swap=True), want_sw, "swapped")
    assert np.array_equal(want_sw[:, 2] == -3, c.expect_invalid())
