"""Test infrastructure of the surfaces from the integer-class kernels (mimc3_match_ncc_full_surf, mimc3_stack_add_class): the fixtures
the CPU and GPU tests share -- the makers of tests/*_common.py at the grids and null fractions at which every form of every kernel
finishes at least two points -- the count of those forms' points on the CPU, and the surface contract of include/mimc3_hip.h."""
import numpy as np

from full_dn_common import dn16_case
from full_multi_common import parity_case
from full_planes_common import dn12_case

BITS = (8, 12, 16)
PATH = {8: "u8_mfma_full", 12: "u16_full", 16: "f32i_full"}
SURF_OCW = (7, 16, 40)                  # the smallest chip, the benchmark's, the largest LDS carve
SURF_R = (1, 4, 15)                     # S = 3, 9, 31 against the 32-wide tile
# (null fraction, dimx, dimy) of the null fixture per chip size: chosen so that null_classes() finds >= 2 points of every class at every
# R of SURF_R, both ways round (test_full_surf_cpu.py asserts it without a device)
NULL_GRID = {7: (0.04, 7, 6), 16: (0.03, 5, 4), 40: (0.01, 8, 6)}


def surf_case(bits, ocw, nulls, radius):
    """The pair and grid of one case -> (case, i0, i1, a-priori shift); nulls False: the null-free pair on the 5 x 4 grid"""
    frac, dimx, dimy = NULL_GRID[ocw] if nulls else (0.0, 5, 4)
    if bits == 8:
        c, shift = parity_case(ocw, frac, radius, dimx=dimx, dimy=dimy)
        return c, c.i0, c.i1, shift
    return (dn12_case if bits == 12 else dn16_case)(ocw, frac, radius, dimx=dimx, dimy=dimy)


def null_classes(i0, i1, xy, offset, shift, ocw, radius, swap=False):
    """Per point the form that finishes it, as the kernels decide: 0 no null in the chip or in the search box, 1 nulls in the box only,
    2 nulls in the chip.  The chip comes from i0 (swap: i1) around uv0, the box of half-width ocw + radius from the other image around
    uv0 + offset + shift; box pixels outside the image are the planes' zero border, i.e. nulls.  (The 8-bit kernel distinguishes all
    three; the u16 and f32 kernels 0 -- clean -- from 1 and 2 -- dirty.)"""
    a, b = (i1, i0) if swap else (i0, i1)
    H, W = a.shape
    h = ocw + radius
    cls = np.zeros(xy.shape[0], np.int32)
    for g in range(xy.shape[0]):
        u, v = int(xy[g, 2]), int(xy[g, 3])
        cu = u + int(offset[0]) + (0 if shift is None else int(shift[g, 0]))
        cv = v + int(offset[1]) + (0 if shift is None else int(shift[g, 1]))
        chip = a[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1]
        box = np.zeros((2 * h + 1, 2 * h + 1), np.float32)
        y0, y1, x0, x1 = max(cv - h, 0), min(cv + h + 1, H), max(cu - h, 0), min(cu + h + 1, W)
        if y1 > y0 and x1 > x0:
            box[y0 - (cv - h):y1 - (cv - h), x0 - (cu - h):x1 - (cu - h)] = b[y0:y1, x0:x1]
        cls[g] = 2 if (chip == 0).any() else (1 if (box == 0).any() else 0)
    return cls


def class_counts(cls):
    return tuple(int((cls == k).sum()) for k in range(3))


def every_form_stores(bits, cls, least=2):
    """True when every form the class's kernel distinguishes finishes at least `least` points"""
    n = class_counts(cls)
    return min(n) >= least if bits == 8 else (n[0] >= least and n[1] + n[2] >= least)


def surfaces_equal(got, want, what=""):
    """The surface contract: cell for cell the same f32 values -- finite cells bit for bit, a non-finite cell of the same kind (NaN, +Inf
    or -Inf); NaN payload bits are not part of it.  -> True when the two arrays are also equal byte for byte"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), f"{what}: NaN masks differ at {np.argwhere(ng != nw)[:5].tolist()}"
    gi, wi = np.where(ng, 0, got).view(np.uint32), np.where(nw, 0, want).view(np.uint32)      # (+-Inf and -0.0 compare by their bits)
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} cells differ, first {bad[:5].tolist()} {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"
    return got.tobytes() == want.tobytes()
