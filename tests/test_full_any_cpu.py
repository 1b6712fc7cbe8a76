"""CPU: the interface of the exhaustive search on any f32 pair (mimc3_match_ncc_full_any), and its test-side oracle
(tests/full_any_oracle.c): against tests/full_dn_oracle.c on the integer classes, against a Python restatement of the reference's two
null rules on NaN, negative, -0.0 and tiny pixels and against a one-pivot DLC match of the pinned oracle (oracle/oracle.py) and of the
compiled reference on the same nine cells, and -- the bound of include/mimc3_hip.h with the reference arithmetic alone -- its two
summation orders against each other on every float fixture the GPU tests use, plus a wide-range fixture on which the order shows."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import (APART_OCW, APART_R, ENCODINGS, FILTERED_KERNELS, FILTERED_OCW, FILTERED_R, cli_kernels, float_case, full_any,
                             null_rule_pair, rules_apart_case, surface_distance, tail_from_surface, wide_case)
from full_dn_common import dn16_case, full_dn, periodic_pair16, status_case16
from full_multi_common import STATUS_R, parity_case
from full_planes_common import PLANES_OCW, PLANES_R, dn12_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mimc3_match_ncc_full_any", "mimc3_match_ncc_full_any_dev")
MIN_DN = 1e-10


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared in mimc3_hip.h"
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"


def check_equals_full_dn(i0, i1, xy, off, ocw, radius, shift, swap, what):
    want_rec, want_cand, want_nlm, want_surf = full_dn(i0, i1, xy, off, ocw, radius, 8, shift=shift, swap=swap, with_counts=True,
                                                       with_surface=True)
    for order in (0, 1):            # exact sums: the order cannot show
        rec, cand, surf, nlm = full_any(i0, i1, xy, off, ocw, radius, 8, shift=shift, swap=swap, order=order)
        assert_bits_equal(surf, want_surf, f"{what}: surface, order {order}")
        assert_bits_equal(rec, want_rec, f"{what}: record, order {order}")
        assert_bits_equal(cand, want_cand, f"{what}: candidates, order {order}")
        assert np.array_equal(nlm, want_nlm)
    # the tail as a function of the surface: the oracle's own
    st3 = want_rec[:, 2] == -3
    rec2, cand2 = tail_from_surface(want_surf, shift, radius, 8, refused=st3)
    assert_bits_equal(rec2, want_rec, f"{what}: tail_from_surface record")
    assert_bits_equal(cand2, want_cand, f"{what}: tail_from_surface candidates")


@pytest.mark.parametrize("ocw,radius", [(7, 7), (16, 15), (30, 1), (40, 7)])
def test_oracle_equals_full_dn_on_the_integer_classes(ocw, radius):
    c, i0, i1, shift = dn16_case(ocw, 0.03, radius)
    check_equals_full_dn(i0, i1, c.xyuvav, c.offset, ocw, radius, shift, False, f"16-bit ocw {ocw}")
    check_equals_full_dn(i0, i1, c.xyuvav, -c.offset, ocw, radius, -shift, True, f"16-bit ocw {ocw} swapped")
    c, i0, i1, shift = dn12_case(ocw, 0.03, radius)
    check_equals_full_dn(i0, i1, c.xyuvav, c.offset, ocw, radius, shift, False, f"12-bit ocw {ocw}")
    c, shift = parity_case(ocw, 0.0, radius, dimx=5, dimy=4)
    check_equals_full_dn(c.i0, c.i1, c.xyuvav, c.offset, ocw, radius, shift, False, f"8-bit ocw {ocw}")


def test_oracle_equals_full_dn_on_statuses_and_ties():
    i0, i1, xy = status_case16()
    check_equals_full_dn(i0, i1, xy, (0, 0), 7, STATUS_R, None, False, "statuses")
    p0, p1, pxy = periodic_pair16()
    check_equals_full_dn(p0, p1, pxy, (0, 0), 15, 15, None, False, "ties")


# ---- the two null rules, restated from MIMC_module.c:622, :631, :723 ----
def cell_py(a, b):
    """(:719-734) on float32 [cw][cw] chips: columns outer, rows inner."""
    n = 0.0
    sx = sy = sxx = syy = sxy = np.float64(0.0)
    cw = a.shape[0]
    for c in range(cw):
        for r in range(cw):
            pa, pb = a[r, c], b[r, c]
            if np.float64(pa) >= MIN_DN and np.float64(pb) >= MIN_DN:           # :723
                n += 1.0
                sx += np.float64(pa); sy += np.float64(pb)
                sxx += np.float64(np.float32(pa * pa)); syy += np.float64(np.float32(pb * pb)); sxy += np.float64(np.float32(pa * pb))
    n = np.float64(n)
    with np.errstate(all="ignore"):
        return np.float32((n * sxy - sx * sy) / np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy)))


def point_py(i0, i1, u0, v0, ocw, R):
    """One point at offset (0, 0), its box inside the image -> (refused, float32[S * S] surface in k order)."""
    chip = i0[v0 - ocw:v0 + ocw + 1, u0 - ocw:u0 + ocw + 1]
    h = ocw + R
    box = i1[v0 - h:v0 + h + 1, u0 - h:u0 + h + 1]
    bad_chip = int((chip.astype(np.float64) < MIN_DN).sum())                    # :622
    bad_box = int((box.astype(np.float64) < MIN_DN).sum())                      # :631
    refused = bool(np.float32(bad_chip) / np.float32(chip.size) > np.float32(0.8) or np.float32(bad_box) / np.float32(box.size) > np.float32(0.8))
    S = 2 * R + 1
    val = np.full(S * S, np.nan, np.float32)
    if not refused:
        cw = 2 * ocw + 1
        for x in range(S):
            for y in range(S):
                val[x * S + y] = cell_py(chip, box[y:y + cw, x:x + cw])
    return refused, val


def test_null_rules_against_python():
    i0, i1, xy = null_rule_pair()
    ocw, R = 7, 2
    rec, _, surf, _ = full_any(i0, i1, xy, (0, 0), ocw, R, 0)
    seen = set()
    for g in range(xy.shape[0]):
        refused, val = point_py(i0, i1, int(xy[g, 2]), int(xy[g, 3]), ocw, R)
        assert refused == (rec[g, 2] == -3), g
        assert_bits_equal(surf[g], val, f"point {g}")
        seen.add("refused" if refused else ("no_cell" if not np.isfinite(val).any() else "cells"))
    assert seen == {"refused", "no_cell", "cells"}
    assert rec[1, 2] == -2 and rec[2, 2] == -3
    # what full_dn_oracle.c's single rule (p < MIN_DN -> skip) would do on NaN differs: the fixture tells the rules apart
    old = full_dn(i0, i1, xy, (0, 0), ocw, R, 0, with_surface=True)[2]
    assert not np.array_equal(np.isfinite(old[0]), np.isfinite(surf[0])) or not np.array_equal(old[0].view(np.uint32), surf[0].view(np.uint32))


def dlc_one_pivot(orc, i0, i1, xy, ocw):
    """A DLC match with the single pivot (0, 0) and offset (0, 0): the climb evaluates the 3 x 3 cells around the centre (the cells of
    the search at R = 1) and, where the centre is their maximum, stops there and fits them -> float32[N][3] (du, dv, ncc)."""
    n = xy.shape[0]
    return orc.match(i0, i1, xy, (0, 0), np.arange(n + 1, dtype=np.int64), np.zeros((n, 2), np.int32), ocw)


def check_against_dlc(orc, i0, i1, xy, ocw, what):
    """Where the search at R = 1 has a fit (its peak is the centre cell), its (du, dv, ncc_peak) are the one-pivot DLC match's, bit for
    bit: the same nine cells under the same two null rules, the same fit.  A chip without an included pixel is (NaN, NaN, -2) on both
    sides; a chip the validity rule refuses is -3 on both (the DLC's search area is two pixels wider and its last row and column are
    zeros, so only the chip's side of the rule is comparable).  -> the set of statuses compared"""
    rec = full_any(i0, i1, xy, (0, 0), ocw, 1, 0)[0]
    dlc = dlc_one_pivot(orc, i0, i1, xy, ocw)
    seen = set()
    for g in range(xy.shape[0]):
        st = rec[g, 2]
        if st >= -1 or st == -2:
            assert_bits_equal(rec[g:g + 1, :3], dlc[g:g + 1], f"{what}: point {g} vs the one-pivot DLC match")
            seen.add("fit" if st >= -1 else "-2")
        elif st == -3:
            u, v = int(xy[g, 2]), int(xy[g, 3])
            chip = i0[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1].astype(np.float64)
            if np.float32((chip < MIN_DN).sum()) / np.float32(chip.size) > np.float32(0.8):
                assert dlc[g, 2] == -3, f"{what}: point {g}"
                seen.add("-3")
    return seen


def centred(i0, i1):
    """i1 with every pixel that is plainly valid in both images replaced by i0's plus a little noise (the peak of the nine cells is the
    centre one wherever the chip has texture left); i1's excluded and tiny pixels stay where they are."""
    out = np.array(i1, np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        m = (i0 >= 1e-8) & (i1 >= 1e-8) & np.isfinite(i0) & np.isfinite(i1)
    out[m] = i0[m] + np.float32(0.5) * (i1[m] - np.floor(i1[m]))
    return out


def dlc_cases():
    i0, i1, xy = null_rule_pair()
    n0, m0, f1, _, axy = rules_apart_case()
    return [("null_rule_pair", i0, centred(i0, i1), xy, 7), ("NaN chip", n0, centred(n0, f1), axy, APART_OCW),
            ("-9999 chip", m0, centred(m0, f1), axy, APART_OCW)]


def test_null_rules_against_the_pinned_oracle(oracle):
    """tests/test_null_encodings_oracle.py pins oracle/oracle.py to the compiled reference on NaN, negative, -0.0 and sub-1e-10 pixels;
    this ties full_any_oracle.c's two null rules to it."""
    seen = set()
    for what, i0, i1, xy, ocw in dlc_cases():
        seen |= check_against_dlc(oracle, i0, i1, xy, ocw, what)
    assert seen == {"fit", "-2", "-3"}, seen


def test_null_rules_against_the_compiled_reference(reference):
    seen = set()
    for what, i0, i1, xy, ocw in dlc_cases():
        seen |= check_against_dlc(reference, i0, i1, xy, ocw, what)
    assert seen == {"fit", "-2", "-3"}, seen


# ---- the bound holds with the reference arithmetic alone: every float fixture tests/test_full_any.py uses ----
BOUND = 6560 * 2.0 ** -53                # (m - 1) 2^-53 for m = 6,561 terms: include/mimc3_hip.h


def check_orders(f0, f1, xy, off, ocw, radius, shift, swap, what):
    """The oracle's two summation orders: the same finite mask, every finite cell within 1 f32 ulp, every sum within the header's bound
    of the other order's (twice the bound on each against the exact sum).  -> share of the cells with a sum whose f64 bits differ"""
    a = full_any(f0, f1, xy, off, ocw, radius, 0, shift=shift, swap=swap, order=0, with_sums=True)
    b = full_any(f0, f1, xy, off, ocw, radius, 0, shift=shift, swap=swap, order=1, with_sums=True)
    share, worst = surface_distance(b[2], a[2], what)
    sa, sb = a[4], b[4]
    assert np.array_equal(sa[..., 0], sb[..., 0]), what + ": n"
    ok = np.isfinite(sa).all(axis=-1) & np.isfinite(sb).all(axis=-1) & (sa[..., 0] > 0)
    with np.errstate(all="ignore"):
        rel = np.abs(sa - sb)[ok][:, 1:] / np.abs(sa)[ok][:, 1:]
    inexact = float((rel > 0).any(axis=1).mean()) if ok.any() else 0.0
    print(f"{what}: {share:.5f} of the finite cells differ between the two orders, at most {worst} ulp; {inexact:.4f} of the cells have "
          f"a sum whose f64 bits differ, by at most {rel.max() if rel.size else 0.0:.3g} (relative)")
    assert worst <= 1, what
    assert rel.size == 0 or rel.max() <= 2 * BOUND, what
    return inexact


@pytest.mark.parametrize("radius", PLANES_R)
@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_float_fixtures_satisfy_the_bound(ocw, encoding, radius):
    """test_full_any.py::test_float_pair's fixtures.  Their f32 terms lie between 2^-3 and 2^14, at most 6,561 of them: every f64
    partial sum is exact in any order (asserted: no sum differs), so on these the bound holds trivially."""
    c, f0, f1, shift = float_case(ocw, 0.03, radius, encoding)
    for swap in (False, True):
        sgn = -1 if swap else 1
        assert check_orders(f0, f1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap,
                            f"ocw {ocw} R {radius} {encoding} swap {swap}") == 0.0


@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_float_fixtures_without_nulls_satisfy_the_bound(ocw):
    c, f0, f1, shift = float_case(ocw, 0.0, 15, "zero")
    check_orders(f0, f1, c.xyuvav, c.offset, ocw, 15, shift, False, f"ocw {ocw} no nulls R 15")
    check_orders(f0, f1, c.xyuvav, c.offset, ocw, 7, None, False, f"ocw {ocw} no nulls R 7 no shift")


def test_rules_apart_fixtures_satisfy_the_bound():
    n0, m0, f1, f1i, xy = rules_apart_case()
    for what, a, b in (("NaN chip, Inf box", n0, f1i), ("NaN chip", n0, f1), ("-9999 chip", m0, f1)):
        check_orders(a, b, xy, (0, 0), APART_OCW, APART_R, None, False, what)


@pytest.mark.parametrize("ocw", FILTERED_OCW)
def test_filtered_float_fixtures_satisfy_the_bound(oracle, ocw):
    """test_full_any.py::test_filtered_float_pair's pairs, filtered on the CPU (GMA_float_conv2 as the pinned oracle restates it); the GPU
    test repeats the check on the pair the device filtered."""
    c, f0, f1, shift = float_case(ocw, 0.03, FILTERED_R, "zero")
    for k in FILTERED_KERNELS:
        kern = np.asarray(cli_kernels()[k], np.float32)
        g0, g1 = oracle.float_conv2(f0, kern), oracle.float_conv2(f1, kern)
        check_orders(g0, g1, c.xyuvav, c.offset, ocw, FILTERED_R, shift, False, f"filtered, kernel {k}, ocw {ocw}")


@pytest.mark.parametrize("radius,encoding", [(7, "zero"), (15, "nan_zero"), (15, "m9999_nan")])
@pytest.mark.parametrize("ocw", PLANES_OCW)
def test_wide_range_fixtures_satisfy_the_bound(ocw, radius, encoding):
    """A fixture on which the order DOES show: six decades of amplitude make the f64 partial sums inexact (asserted at the two large
    chips: nearly every cell has a sum whose last bits depend on the order), within the header's bound, and the f32 cells stay
    within 1 ulp."""
    c, f0, f1, shift = wide_case(ocw, 0.03, radius, encoding)
    inexact = check_orders(f0, f1, c.xyuvav, c.offset, ocw, radius, shift, False, f"wide ocw {ocw} R {radius} {encoding}")
    if ocw >= 30:
        assert inexact > 0.5
