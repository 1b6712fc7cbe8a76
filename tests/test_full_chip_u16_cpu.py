"""CPU: what the GPU tests of the exhaustive search on scaled-integer pairs at any chip size on the matrix cores
(tests/test_full_chip_u16.py) rest on, without a device.

  * the new symbols are declared in the header and exported by the library, path 13 has its name; the layout in Python terms is the
    library's, fits a compute unit's LDS at every ocw, and has the boundary chip sizes the GPU tests derive from it;
  * every fixture a GPU test uses, counted in numpy: the null pattern of every point, and many distinct values in each 6-bit plane;
  * the plane recombination of sum ab, the byte-plane splits of the box sums and every integer bound the kernel states, in integer numpy
    on a saturated CW-161 case;
  * on the saturated fixtures ONE packed u16 table query of a chip is right at ocw 44 and wrong at ocw 45, the 64 x 64 cut right at both;
  * on the saturated fixtures no product of the finish exceeds 2^53 at ocw 75 and some do at ocw 76 and 80: the rounding cases of the
    finish are really exercised by the GPU cases there."""
import os
import re

import numpy as np
import pytest

import full_chip_u16_common as fp
import value_limit_common as vl
from conftest import ROOT

SYMBOLS = ("mimc3_match_ncc_full_chip_planes", "mimc3_match_ncc_full_chip_planes_dev", "mimc3_full_chip_planes_layout")


def test_symbols_are_declared_and_exported():
    from mimc3_amd import api
    header = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/mimc3_hip.h"
        assert getattr(api._lib, name) is not None
    assert " 13 = " in header and '13: "u16_mfma_chip"' in open(os.path.join(ROOT, "mimc3_amd", "api.py")).read()
    for name in ("match_ncc_full_chip_planes", "match_ncc_full_chip_planes_dev"):
        assert hasattr(api.Context, name)
    assert hasattr(api, "full_chip_planes_layout")


def test_layout_is_the_librarys_and_fits():
    from mimc3_amd import api
    for ocw in range(0, fp.MAX_OCW + 2):
        assert api.full_chip_planes_layout(ocw) == fp.layout_tuple(ocw), ocw
    for ocw in range(1, fp.MAX_OCW + 1):
        L = fp.layout(ocw)
        assert 1 <= L["KCW"] <= 3 and L["KCW"] == -(-(L["CW"] + 15) // 64)
        assert L["NTR"] <= 12 and L["KCV"] <= 3 and L["lds"] <= 160 * 1024
    assert 2 * fp.layout(56)["lds"] <= 160 * 1024 < 2 * fp.layout(57)["lds"]       # two workgroups per CU up to the two-chunk class
    b = fp.boundaries()
    assert b["KCW"] == [(24, 25), (56, 57)]
    assert b == fp.boundaries(api.full_chip_planes_layout)
    sizes = [o for o, _ in fp.size_cases()]
    assert {1, 2, 3, 10, 11, 14, 24, 25, 56, 57, 60, 80} <= set(sizes)


def test_integer_bounds():
    cw = 2 * fp.MAX_OCW + 1
    assert cw * cw * 63 * 63 == 102880449 < 2 ** 27                      # a plane correlation
    assert cw * cw * 126 * 126 == 411521796 < 2 ** 29                    # the (h + l) form
    assert 2 ** 31 < cw * cw * 4095 * 4095 == 434669897025 < 2 ** 39     # the true sum ab: not an i32
    assert cw * 4095 == 659295 < 2 ** 20                                 # a row-box sum of q
    assert 2 ** 31 < cw * 4095 * 4095 == 2699813025 < 2 ** 32            # a row-box sum of q^2
    sq = vl.sat_shifts()["kSatSqShift16"]
    assert 64 * 64 * 4095 < 2 ** sq and 64 * 64 * 4095 ** 2 < 2 ** (64 - sq)
    assert 89 * 89 * 4095 < 2 ** sq <= 91 * 91 * 4095                    # ocw 44 | 45
    assert 8194 * 4095 < 2 ** sq <= 8195 * 4095                          # (8,193 saturated pixels are safe, 8,195 are not)


@pytest.mark.parametrize("ocw,radius,kind,swap,with_shift", fp.all_fixtures())
def test_fixture_counts(ocw, radius, kind, swap, with_shift):
    c, i0, i1, shift = fp.u16_case(ocw, radius, kind, "placed", swap, with_shift)
    assert 12 <= c.n <= 20
    q0, q1 = fp.integers(kind, i0, i1)
    nc, nb = fp.null_counts(c, i0, i1, shift, ocw, radius, swap)
    clean, box_only, chip_only, both = (nc == 0) & (nb == 0), (nc == 0) & (nb > 0), (nc > 0) & (nb == 0), (nc > 0) & (nb > 0)
    assert list(np.flatnonzero(box_only)) == list(fp.BOX_ONLY) and list(np.flatnonzero(chip_only)) == list(fp.CHIP_ONLY)
    assert list(np.flatnonzero(both)) == list(fp.BOTH) and clean.sum() == 6
    for q in (q0, q1):
        h, l = np.unique(q[q > 0] >> 6).size, np.unique(q[q > 0] & 63).size
        if kind.startswith("sat"):                                      # pressed against 4095: the low plane carries the spread
            assert l >= (3 if kind == "sat3" else 24), (kind, h, l)
        else:
            assert h >= 16 and l >= 48, (kind, h, l)


def test_the_other_null_patterns():
    c, i0, i1, shift = fp.u16_case(10, 7, "dn12", "none")
    nc, nb = fp.null_counts(c, i0, i1, shift, 10, 7, False)
    assert not nc.any() and not nb.any()
    c, i0, i1, shift = fp.u16_case(10, 7, "dn12", "all")
    nc, nb = fp.null_counts(c, i0, i1, shift, 10, 7, False)
    assert (nb > 0).all() and (nc > 0).sum() >= 2 and (nc == 0).sum() >= 2


def byte_planes(x, n):
    return [(x >> (8 * k)) & 255 for k in range(n)]


def test_plane_arithmetic_on_a_saturated_cw161_case():
    """the kernel's integer route for one cell of every point at ocw 80: q = 64 h + l, three plane correlations, row-box sums split into
    byte planes in offset form, against the direct sums"""
    ocw, R = 80, 15
    cw = 2 * ocw + 1
    for kind in ("sat3", "sat63"):
        c, i0, i1, shift = fp.u16_case(ocw, R, kind, "none")
        q0, q1 = fp.integers(kind, i0, i1)
        u, v, cu, cv = fp.geometry(c, shift, False)
        for g in (0, 5, 11):
            a = q0[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
            b = q1[cv[g] - ocw:cv[g] + ocw + 1, cu[g] - ocw:cu[g] + ocw + 1]
            ah, al, bh, bl = a >> 6, a & 63, b >> 6, b & 63
            assert ah.max() <= 63 and (ah + al).max() <= 126
            HH, LL, SS = int((ah * bh).sum()), int((al * bl).sum()), int(((ah + al) * (bh + bl)).sum())
            assert HH < 2 ** 27 and LL < 2 ** 27 and SS < 2 ** 29
            sab = int((a * b).sum())
            assert 4096 * HH + 64 * (SS - HH - LL) + LL == sab and 2 ** 31 < sab < 2 ** 39
            # row-box sums of q: three byte planes; of q^2: a u32, four; the signed bytes x - 128 summed over cw rows, + 128 cw per plane
            rq, rqq = b.sum(axis=1), (b * b).sum(axis=1)
            assert rq.max() < 2 ** 20 and 2 ** 31 < rqq.max() < 2 ** 32
            for r, n in ((rq, 3), (rqq, 4)):
                tot = sum(256 ** k * (int((p - 128).sum()) + 128 * cw) for k, p in enumerate(byte_planes(r, n)))
                assert tot == int(r.sum())
            assert int(rqq.sum()) < 2 ** 39
            # q^2 of a pixel: three byte planes
            assert (a * a).max() < 2 ** 24 and sum(256 ** k * p for k, p in enumerate(byte_planes(a * a, 3))).sum() == (a * a).sum()


@pytest.mark.parametrize("kind", ["sat3", "sat63"])
def test_one_packed_query_fails_at_45_and_not_at_44(kind):
    sq = vl.sat_shifts()["kSatSqShift16"]
    for ocw, whole_is_right in ((44, True), (45, False)):
        c, i0, i1, shift = fp.u16_case(ocw, 15, kind, "placed")
        q = fp.integers(kind, i0, i1)[0]
        cw = 2 * ocw + 1
        S = vl.table(vl.pack_u16(q, sq))
        u, v = vl.grid_uv(c.xyuvav)
        y, x = v - ocw, u - ocw
        true = [vl.box_sums(vl.table(w), cw, cw)[y, x].astype(np.int64) for w in (q, q * q)]
        whole = [f[y, x].astype(np.int64) for f in vl.unpack_u16(vl.box_sums(S, cw, cw), sq)]
        split = [np.zeros(c.n, np.int64) for _ in range(2)]
        for j in range(0, cw, 64):
            for i in range(0, cw, 64):
                w0, h0 = min(cw - i, 64), min(cw - j, 64)
                for k, f in enumerate(vl.unpack_u16(vl.box_sums(S, w0, h0), sq)):
                    split[k] += f[y + j, x + i].astype(np.int64)
        for k in range(2):
            assert np.array_equal(split[k], true[k]), (ocw, k)
        right = all(np.array_equal(whole[k], true[k]) for k in range(2))
        assert right == whole_is_right, f"{kind} ocw {ocw}: one packed query is {'right' if right else 'wrong'}"


def finish_products(kind, ocw):
    """the largest of the finish's six products (n sxy, sx sy, n sxx, sx^2, n syy, sy^2) over the clean points, at the search centre"""
    c, i0, i1, shift = fp.u16_case(ocw, 15, kind, "placed")
    q0, q1 = fp.integers(kind, i0, i1)
    u, v, cu, cv = fp.geometry(c, shift, False)
    nc, nb = fp.null_counts(c, i0, i1, shift, ocw, 15, False)
    top = 0
    for g in np.flatnonzero((nc == 0) & (nb == 0)):
        a = q0[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
        b = q1[cv[g] - ocw:cv[g] + ocw + 1, cu[g] - ocw:cu[g] + ocw + 1]
        n, sx, sy, sxx, syy, sxy = a.size, int(a.sum()), int(b.sum()), int((a * a).sum()), int((b * b).sum()), int((a * b).sum())
        top = max(top, n * sxy, sx * sy, n * sxx, sx * sx, n * syy, sy * sy)
    return top


def test_the_finish_rounds_from_ocw_76_on():
    for kind in ("sat3", "sat63"):
        t75, t76, t80 = (finish_products(kind, o) for o in (75, 76, 80))
        print(f"{kind}: largest product / 2^53 at ocw 75: {t75 / 2 ** 53:.4f}, 76: {t76 / 2 ** 53:.4f}, 80: {t80 / 2 ** 53:.4f}")
        assert t75 < 2 ** 53 < t76 < t80
