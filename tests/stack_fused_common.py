"""Fixtures of the fused stack layers (mimc3_stack_add_fused: the accumulating forms of the run-time-ocw matrix-core searches) that the
CPU and GPU tests share: the (ocw, R) tables -- the smallest shapes at which each form can go wrong -- the radius limits per pixel class
restated from the library's existing queries, and pairs with PLACED nulls on a 6 x 4 grid whose search boxes do not overlap
(full_chip_u8_common's construction with more points): two points with a null in the box only, two in the chip only, two on both sides,
one refused (its chip is all null: status -3), seventeen clean.  Three layers per case: raw, swapped, another chip size."""
import functools

import numpy as np

import full_chip_u8_common as fu
from full_any_common import full_any
from full_chip_u16_common import spread12
from stack_common import NumpyStack, refused_of

FINISHES = ((4, 1), (0, 2), (8, 3))                     # (npeaks, min_count) of every comparison
WHAT = ("record", "candidates", "count", "mean surface")
SIX = fu.SIX
DIMX, DIMY = 6, 4
BOX_ONLY, CHIP_ONLY, BOTH, REFUSED = (0, 1), (2, 3), (4, 5), 6


def _entry_exists():
    """every test of the two files needs the entries: without them they fail here, at the missing symbol"""
    from mimc3_amd import api
    return api._lib.mimc3_stack_fused_max_radius is not None and hasattr(api.Context, "stack_add_fused")


assert _entry_exists()

# (ocw, R, the chip size of the third layer).  8-bit pair: one, two and three K chunks per chip row up to R 15; 2 x 2 cell tiles (S = 33),
# 3 x 3 with a last partial tile (S = 67), the largest radius, the largest chip
U8_CASES = ((10, 4, 7), (10, 15, 12), (25, 15, 24), (57, 8, 56), (16, 15, 15), (7, 16, 9), (7, 33, 5), (16, 47, 7), (80, 16, 60))
# 12-bit pair and d/dx-filtered 8-bit pair: ocw 80 at its largest radius
U16_CASES = ((10, 15, 12), (16, 20, 15), (45, 8, 44), (80, 27, 60))
ORACLE_CASES = (("u8", 10, 4, 7), ("u8", 7, 16, 9), ("dn12", 10, 15, 12))
PATHS = {"u8": ("u8_mfma_chip", "u8_mfma_wide"), "dn12": ("u16_mfma_chip", "u16_mfma_wide"), "ddx": ("u16_mfma_chip", "u16_mfma_wide")}


def path_of(kind, R):
    return PATHS[kind][0 if R <= 15 else 1]


def max_radius(kind, ocw, api):
    """The largest stack radius the entry takes, from the library's EXISTING queries: 47 on an 8-bit pair; wide_planes_max_radius(ocw) on a
    scaled-integer one; 15 on any other, or wide_max_radius(ocw) at the six chip sizes.  0 outside 1..80"""
    if not 1 <= ocw <= 80:
        return 0
    if kind == "u8":
        return 47
    if kind in ("dn12", "ddx"):
        return api.wide_planes_max_radius(ocw)
    return max(15, api.wide_max_radius(ocw)) if ocw in SIX else 15


@functools.lru_cache(maxsize=None)
def _base(ocw, R):
    """full_chip_u8_common._base with 6 x 4 points: a null-free 8-bit pair and a grid whose boxes lie 2 (ocw + R) + 15 px apart"""
    from mimc3_amd import api, synth
    h = ocw + R
    step, margin = 2 * h + 15, h + 12
    c = synth.make_small(seed=7400 + ocw, shift=(3, -2), angle_deg=40.0, ocw=ocw, speed=700.0, h=2 * margin + (DIMY - 1) * step + 1,
                         w=2 * margin + (DIMX - 1) * step + 1, dimx=DIMX, dimy=DIMY, noise_dn=2, null_frac=0.0, offset=(1, -1), sigma=0.3,
                         margin=margin)
    i0, i1 = np.where(c.i0 == 0, 1, c.i0).astype(np.float32), np.where(c.i1 == 0, 1, c.i1).astype(np.float32)
    shift = np.ascontiguousarray(api.prior_shift(c.xyuvav, c.dt, c.mpp), np.int32)
    return c, i0, i1, shift


@functools.lru_cache(maxsize=4)
def fixture(ocw, R, kind="u8", nulls="placed"):
    """-> dict(c, i0, i1, xy, off, shift, ocw, R, kind).  kind: "u8", "dn12" (spread12 of the 8-bit pair, the nulls placed afterwards);
    nulls: "placed", "all" (every point holds a null: none is the clean form's), "refused" (every chip is all null)"""
    c, b0, b1, shift = _base(ocw, R)
    i0, i1 = (b0.copy(), b1.copy()) if kind == "u8" else (np.array(spread12(b0), np.float32), np.array(spread12(b1), np.float32))
    u, v, cu, cv = fu.geometry(c, shift, False)
    h = ocw + R
    if nulls == "placed":
        g = BOX_ONLY[0]; i1[cv[g] + h, cu[g] - 3] = 0                   # the last box row
        g = BOX_ONLY[1]; i1[cv[g] + 2, cu[g] + h] = 0                   # the last box column
        g = CHIP_ONLY[0]; i0[v[g] - ocw, u[g]] = 0                      # the first chip row
        g = CHIP_ONLY[1]; i0[v[g] + ocw, u[g] + ocw] = 0                # the last chip row (and column)
        g = BOTH[0]; i0[v[g], u[g] - 1] = 0; i1[cv[g] + 1, cu[g]] = 0
        g = BOTH[1]; i0[v[g] - 1, u[g] - ocw] = 0; i1[cv[g] - h, cu[g] + 1] = 0
        g = REFUSED; i0[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 0
    elif nulls == "all":
        for g in range(c.n):
            i1[cv[g] - h + (7 * g) % (2 * h + 1), cu[g] + h - (5 * g) % (2 * h + 1)] = 0
            if g & 1:
                i0[v[g] + ocw - (3 * g) % (2 * ocw + 1), u[g] - ocw + (11 * g) % (2 * ocw + 1)] = 0
    else:
        assert nulls == "refused"
        for g in range(c.n):
            i0[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 0
    f = dict(c=c, i0=np.ascontiguousarray(i0, np.float32), i1=np.ascontiguousarray(i1, np.float32), xy=np.ascontiguousarray(c.xyuvav, np.float64),
             off=np.ascontiguousarray(c.offset, np.int32), shift=shift, ocw=ocw, R=R, kind=kind, what=f"{kind} ocw {ocw} R {R} nulls {nulls}")
    for a in (f["i0"], f["i1"], f["xy"], f["off"], shift):
        a.setflags(write=False)
    return f


def layers_of(f, ocw2):
    """the three layers (ocw, swap): raw, swapped, another chip size"""
    return ((f["ocw"], False), (f["ocw"], True), (ocw2, False))


def kinds(f):
    """per point of the fixture's first layer, from its pixels alone -> (nulls in the chip, nulls in the box, refused bool)"""
    nc, nb = fu.null_counts(f["c"], f["i0"], f["i1"], f["shift"], f["ocw"], f["R"], False)
    ref = (nc / float((2 * f["ocw"] + 1) ** 2) > 0.8) | (nb / float((2 * (f["ocw"] + f["R"]) + 1) ** 2) > 0.8)
    return nc, nb, ref


def qualifies(f):
    """what the issue asks of every fixture used on the GPU, counted from the pixels"""
    nc, nb, ref = kinds(f)
    ok = ~ref
    return ((ok & (nc == 0) & (nb == 0)).sum() >= 4 and (ok & (nc > 0) & (nb == 0)).sum() >= 2 and (ok & (nc == 0) & (nb > 0)).sum() >= 2 and
            (ok & (nc > 0) & (nb > 0)).sum() >= 2 and ref.sum() >= 1 and 24 <= f["c"].n <= 60)


def oracle_layers(f, ocw2):
    """the CPU oracle's record and surfaces of the three layers"""
    return [full_any(f["i0"], f["i1"], f["xy"], f["off"], ocw, f["R"], 0, shift=f["shift"], swap=swap)[0:3:2] for ocw, swap in layers_of(f, ocw2)]


def oracle_stack(f, ocw2):
    ref = NumpyStack(f["c"].n, f["R"], f["shift"])
    for rec, surf in oracle_layers(f, ocw2):
        ref.add(surf, refused_of(rec))
    return ref


class FusedOrderStack(NumpyStack):
    """NumpyStack fed in the fused order: point by point, each layer's finite cells added once, in add order across the layers"""

    def add_points(self, layers):
        """layers: [(surf, refused)] in add order"""
        for g in range(self.n):
            for surf, refused in layers:
                row = np.asarray(surf[g], np.float32)
                fin = np.isfinite(row)
                self.sum[g, fin] += row[fin].astype(np.float64)
                self.cnt[g, fin] += 1
                if not refused[g]:
                    self.lay[g] += 1
        self.layers += len(layers)
        return self


def same_bytes(a, b, what):
    for x, y, name in zip(a, b, WHAT):
        assert (x is None) == (y is None), f"{what}: {name}"
        if x is not None:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {name}"


def finishes(ctx):
    return [ctx.stack_finish(k, mc, surface=True) for k, mc in FINISHES]
