"""CPU, build container only: the oracle (oracle/mimc3_oracle.c) against the compiled reference on null pixels that are not +0.0
(-0.0, -1, -9999, -inf, NaN of either sign, 1e-11, the largest f32 below 1e-10), on valid pixels at the threshold and +inf, on points
at the 80 % invalid-pixel limit, on the pre-filter's null test at its edges, and on the control-point stage with NaN / -9999 nulls.
Bar: bit for bit (NaN == NaN).  Skipped where oracle/_ref was never built, as test_oracle_vs_ref.py."""
import numpy as np
import pytest

import null_encoding_common as nc
from conftest import assert_bits_equal

MATCH_OCW = (7, 30)


def both_directions(orc, c, off, uv):
    return (orc.match(c.i0, c.i1, c.xyuvav, c.offset, off, uv, c.ocw),
            orc.match(c.i1, c.i0, c.xyuvav, -c.offset, off, -uv, c.ocw))


def compare(oracle, reference, c, what):
    H, W = c.i0.shape
    off, uv = reference.get_uv_pivot(c.xyuvav, c.dt, c.mpp, c.ocw, H, W)
    ref = both_directions(reference, c, off, uv)
    port = both_directions(oracle, c, off, uv)
    assert_bits_equal(port[0], ref[0], what + " forward")
    assert_bits_equal(port[1], ref[1], what + " swapped")
    return ref


@pytest.mark.parametrize("ocw", MATCH_OCW)
@pytest.mark.parametrize("enc", list(nc.ENCODINGS))
def test_match_null_encodings(oracle, reference, enc, ocw):
    c = nc.encoded_case(ocw, enc)
    fw, sw = compare(oracle, reference, c, f"{enc} ocw {ocw}")
    assert np.isfinite(fw[:, 0]).sum() > len(fw) // 2 and np.isfinite(sw[:, 0]).sum() > len(sw) // 2


@pytest.mark.parametrize("ocw", MATCH_OCW)
def test_match_threshold_valued_pixels(oracle, reference, ocw):
    compare(oracle, reference, nc.threshold_case(ocw), f"THR ocw {ocw}")


@pytest.mark.parametrize("ocw", MATCH_OCW)
def test_match_positive_infinity(oracle, reference, ocw):
    fw, sw = compare(oracle, reference, nc.inf_case(ocw), f"+inf ocw {ocw}")
    assert np.isnan(fw[:, 0]).any() and np.isnan(sw[:, 0]).any()          # the +inf pixels reach some points


@pytest.mark.parametrize("ocw", (7, 15, 16, 30, 32, 40))
def test_threshold_pixels_are_not_nulls(oracle, ocw):
    """The GPU tests hold the THR pair to 1e-4 px / 1e-6 NCC: that tolerance must not hide a kernel that treats THR as null.
    Here the same pair with THR replaced by +0.0 moves the oracle's output far beyond it."""
    c = nc.threshold_case(ocw)
    H, W = c.i0.shape
    off, uv = oracle.get_uv_pivot(c.xyuvav, c.dt, c.mpp, c.ocw, H, W)
    a = oracle.match(c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw)
    i0 = np.where(c.i0 == nc.THR, 0, c.i0).astype(np.float32); i1 = np.where(c.i1 == nc.THR, 0, c.i1).astype(np.float32)
    b = oracle.match(i0, i1, c.xyuvav, c.offset, off, uv, ocw)
    same_mask = np.array_equal(np.isnan(a), np.isnan(b))
    assert not same_mask or np.nanmax(np.abs(a[:, :2] - b[:, :2])) > 1e-3 or np.nanmax(np.abs(a[:, 2] - b[:, 2])) > 1e-4


def test_encodings_are_what_they_claim():
    assert float(nc.BELOW_THR) < 1e-10 <= float(nc.THR) and nc.THR == np.nextafter(nc.BELOW_THR, np.float32(1))
    assert np.signbit(nc.ENCODINGS["negzero"]) and np.signbit(nc.ENCODINGS["negnan"]) and not np.signbit(nc.ENCODINGS["nan"])
    assert np.isnan(nc.ENCODINGS["nan"]) and np.isnan(nc.ENCODINGS["negnan"])


@pytest.mark.parametrize("enc", ["zero", "minus1", "nan"])
@pytest.mark.parametrize("ocw", (7, 16, 30, 40))
def test_invalid_limit(oracle, reference, ocw, enc):
    """k - 1, k, k + 1 invalid pixels in the chip and in the search area (its T4 row and column included; written nulls away from
    and on the last written row and column): the point turns -3 exactly at k -- unless the nulls are NaN, which are not counted."""
    c = nc.limit_case(ocw, enc, lambda xy, o, H, W: reference.get_uv_pivot(xy, 16.0, 15.0, o, H, W))
    counts = nc.count_invalid(c)
    counted = enc not in nc.NOT_COUNTED
    t4 = (2 * ocw + 25) + (2 * ocw + 5) - 1
    for (side, n, k), got in zip(c.labels, counts):
        if not counted:
            assert got == (0 if side == "chip" else t4), (side, n, got)
        elif n is not None:
            assert got == n, (side, n, got)
    ref = reference.match(c.chip_img, c.win_img, c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw)
    assert_bits_equal(oracle.match(c.chip_img, c.win_img, c.xyuvav, c.offset, c.piv_off, c.piv_uv, ocw), ref, f"ocw {ocw} {enc}")
    assert np.array_equal(ref[:, 2] == -3, c.expect_invalid(counted)), (ref[:, 2], c.labels)


def test_full_search_limit_counts():
    """The exhaustive search's box (R 7, ocw 16) has no T4 term: the test-side oracle turns -3 exactly at k as well."""
    from full_search_common import full_search
    c = nc.limit_case(16, "zero", radius=7)
    assert [n for _, n, _ in c.labels if n is not None] == nc.count_invalid(c)[:len(c.labels) - 2]
    out = full_search(c.chip_img, c.win_img, c.xyuvav, c.offset, 16, 7)
    assert np.array_equal(out[:, 2] == -3, c.expect_invalid())


def test_conv2_null_test_edges(oracle, reference):
    """(int32_t)(p + 0.5) == 0 at -1.5, nextafter(-1.5, 0), nextafter(0.5, 0), 0.5; NaN; -9999 (valid); 3e9 (out of int32 range:
    INT_MIN on x86-64, "not null" -- DESIGN.md)."""
    c = nc.conv2_case()
    for img in (c.i0, c.i1):
        for v in nc.CONV2_EDGES:
            assert (img.view(np.uint32) == np.float32(v).view(np.uint32)).any()
        for k in nc.CP_KERNELS:
            assert_bits_equal(oracle.float_conv2(img, k), reference.float_conv2(img, k), f"k{k.shape}")


@pytest.mark.parametrize("enc", ["nan", "m9999"])
def test_cp_offset_null_encodings(oracle, reference, enc):
    i0, i1, xy = nc.cp_case(enc)
    for sd in (3, 99):
        a = reference.get_offset_image(i0, i1, xy, nc.CP_KERNELS, sd, num_cp_min=20)
        b = oracle.get_offset_image(i0, i1, xy, nc.CP_KERNELS, sd, num_cp_min=20)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (enc, sd, a[:2], b[:2])
