"""Test infrastructure of the exhaustive search on scaled-integer pairs (12-bit DN, filtered 8-bit pairs) at any chip size on the matrix
cores (mimc3_match_ncc_full_chip_planes, match_full_chip_u16_kernel.hip): the kernel's layout in Python terms, and 12-bit fixtures built
from the placed-null fixtures of tests/full_chip_u8_common.py -- 12 points whose search boxes do not overlap: two with a null in the box
only, two in the chip only, two on both sides, six clean -- with every non-null pixel spread over all twelve bits, so that neither 6-bit
plane of q = 64 h + l is constant or sparse.  tests/test_full_chip_u16_cpu.py counts every fixture without a device."""
import numpy as np

import full_chip_u8_common as fu
from value_limit_common import top_of_class

PATH = "u16_mfma_chip"
MAX_OCW = fu.MAX_OCW
SIX = fu.SIX
BOX_ONLY, CHIP_ONLY, BOTH = fu.BOX_ONLY, fu.CHIP_ONLY, fu.BOTH
KINDS = ("dn12", "sat3", "sat63", "eighths", "mixed")


# ---- the layout (match_full_chip_u16_kernel.hip chip_u16_layout): the u8 kernel's with a second tile and a second chip plane ----
def layout(ocw):
    cw = 2 * ocw + 1
    kw = cw + 31
    kcw = (cw + 15 + 63) // 64
    rdw, sw = 16 + 64 * kcw, (kw + 15) & ~15
    pw0 = max(rdw, sw)
    pw = pw0 if (pw0 // 16) & 1 else pw0 + 16
    ntr = (kw + 15) // 16
    cp = max((cw + 15 + 3) & ~3, 64 * kcw)
    chb = (16 + (cw + 1) * cp + 16 + 15) & ~15
    tb = (max((16 * ntr + 1) * pw, 4 * 32 * 33) + 15) & ~15
    return dict(CW=cw, KCW=kcw, NTR=ntr, KCV=(ntr + 3) // 4, lds=2 * tb + 2 * chb)


def layout_tuple(ocw):
    L = layout(ocw)
    return (L["KCW"], L["NTR"], L["KCV"], L["lds"]) if 1 <= ocw <= MAX_OCW else None


def boundaries(query=layout_tuple):
    return fu.boundaries(query)


def size_cases(query=layout_tuple):
    """(ocw, R): 1, 2, 3, 10, 11, 14, both sides of every change of the layout, 60 and 80 (full_chip_u8_common.size_cases on this layout)"""
    return fu.size_cases(query)


# ---- fixtures ----
def spread12(img8, by_position=True):
    """An 8-bit image (0 = null) as 12-bit DN with all twelve bits varying: a null stays 0, every other pixel p at (x, y) becomes
    16 (p - 1) + 1 + (3 x + 5 y + 7 p) mod 16, in 1 .. 4080.  by_position=False leaves x and y out: a function of p alone, which keeps a
    constant area constant (the status fixtures: -2 needs a window without variance)"""
    p = np.asarray(img8, np.int64)
    y, x = np.indices(p.shape) if by_position else (0, 0)
    q = 16 * (p - 1) + 1 + (3 * x + 5 * y + 7 * p) % 16
    return np.where(p == 0, 0, q).astype(np.float32)


def u16_case(ocw, radius, kind="dn12", nulls="placed", swap=False, with_shift=True):
    """-> (case, i0, i1, shift or None): full_chip_u8_common.u8_case's pair, grid and nulls, its pixels mapped to a scaled-integer class.
    kind: "dn12" spread12; "sat3" / "sat63" pressed against 4095 (top_of_class(..., 4095, 3 | 63): the saturated 12-bit fixtures);
    "eighths" spread12 / 8 on both images (scale 8); "mixed" spread12 / 8 on image 0 alone."""
    c, i0, i1, sh = fu.u8_case(ocw, radius, nulls, swap, with_shift)
    if kind in ("sat3", "sat63"):
        s = int(kind[3:])
        j0, j1 = top_of_class(i0, 4095, s), top_of_class(i1, 4095, s)
    else:
        j0, j1 = spread12(i0), spread12(i1)
        if kind in ("eighths", "mixed"):
            j0 = j0 / np.float32(8)
        if kind == "eighths":
            j1 = j1 / np.float32(8)
        assert kind in ("dn12", "eighths", "mixed")
    return c, np.ascontiguousarray(j0, np.float32), np.ascontiguousarray(j1, np.float32), sh


def integers(kind, i0, i1):
    """the pair as the integers q the u16 planes hold -> two int64 arrays"""
    s0 = 8 if kind in ("eighths", "mixed") else 1
    s1 = 8 if kind == "eighths" else 1
    q0, q1 = i0.astype(np.float64) * s0, i1.astype(np.float64) * s1
    assert np.array_equal(q0, np.rint(q0)) and np.array_equal(q1, np.rint(q1)) and q0.max() < 4096 and q1.max() < 4096
    return q0.astype(np.int64), q1.astype(np.int64)


def filtered_pair(ctx, api, which, i0, i1):
    """The filtered pair: set the 8-bit pair, filter it on the device with the program's kernel `which` (0 d/dx, 1 d/dy, 2 Laplacian) and
    read it back -> the two float images the context now matches on (integers after a gradient, eighths after the Laplacian)"""
    ctx.set_images(i0, i1)
    ctx.filter_images(api.CLI_KERNELS[which])
    f0, f1 = ctx.get_images(*i0.shape)
    assert not np.array_equal(f0, i0)
    return f0, f1


def six_radius(ocw):
    """the radius of the mode-1 cases at the six built chip sizes: 7 at 16 and 32, 15 elsewhere"""
    return 7 if ocw in (16, 32) else 15


null_counts = fu.null_counts
geometry = fu.geometry

# ---- every fixture a GPU test uses: (ocw, R, kind, swap, with_shift) ----
RADII = tuple((o, r) for o in (10, 80) for r in (1, 4, 7, 15))
SATURATED_OCW = (44, 45, 75, 76, 80)


def all_fixtures():
    out = {(o, r, "dn12", False, True) for o, r in size_cases()} | {(o, r, "dn12", False, True) for o, r in RADII}
    out |= {(10, 7, "dn12", True, True), (57, 15, "dn12", True, True), (10, 7, "dn12", False, False), (10, 7, "dn12", True, False)}
    out |= {(o, 15, k, False, True) for o in SATURATED_OCW for k in ("sat3", "sat63")}
    out |= {(o, 7, k, False, True) for o in (10, 60) for k in ("eighths", "mixed")}
    out |= {(o, six_radius(o), "dn12", False, True) for o in SIX}
    return sorted(out)
