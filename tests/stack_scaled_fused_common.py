"""Fixtures of the fused SCALED stack layers (mimc3_stack_add_scaled_fused: the scaled accumulating form of the run-time-ocw matrix-core
searches, stack_acc_scaled) that the CPU and GPU tests share: the case table (pair, ocw, stack R, scale, weight, layer R) -- the smallest
shapes at which each piece can go wrong -- and stack_fused_common's 6 x 4 pairs with placed nulls.

A scaled layer is searched around the LAYER shift Lsh = rint(scale x the stack's shift) at the LAYER radius, so the pair is
stack_fused_common's at (ocw, layer R), and the nulls are placed by its recipe around the layer's box: two points with a null in the box
only, two in the chip only, two on both sides, one refused, seventeen clean (counted from the pixels in the CPU test, on the layer's
view of the fixture).  The stack's shift is chosen per point so that Lsh stays within a few pixels of the pair's prior shift -- the boxes
stay inside the image and apart -- and carries a fixed pattern of odd and negative components, so that scales 0.5 and 2.5 meet ties of
rint that round down and ties that round up.  Three layers per case: raw, swapped (another scale, weight and layer radius), another
chip size."""
import functools

import numpy as np

import full_chip_u8_common as fu
import stack_fused_common as sf
from full_any_common import full_any
from full_chip_u16_common import spread12
from stack_common import refused_of
from stack_scaled_common import NumpyScaledStack, axis_taps, layer_radius, layer_shift

FINISHES, same_bytes, finishes, path_of = sf.FINISHES, sf.same_bytes, sf.finishes, sf.path_of


def _entry_exists():
    """every test of the two files needs the entries: without them they fail here, at the missing symbol"""
    from mimc3_amd import api
    return api._lib.mimc3_stack_add_scaled_fused is not None and api._lib.mimc3_stack_add_scaled_fused_dev is not None and \
        hasattr(api.Context, "stack_add_scaled_fused") and hasattr(api.Context, "stack_add_scaled_fused_dev")


assert _entry_exists()

# (pair, ocw, stack R, scale, weight, layer R, the chip size of the third layer)
CASES = (
    ("u8", 10, 4, 1.0, 1.0, 4, 9),            # 1  must equal stack_add_fused
    ("u8", 10, 4, 2.0, 1.0, 9, 7),            # 2  chip kernel, integer taps
    ("u8", 7, 7, 2.5, 0.3, 19, 5),            # 3  wide kernel with 2 x 2 tiles; the stack turns weighted on this add
    ("u8", 16, 15, 3.0, 1.0, 46, 15),         # 4  wide kernel with 3 x 3 tiles at pitch 96
    ("u8", 7, 33, 0.5, 1.0, 17, 5),           # 5  stack larger than its wide layer: the loop bound
    ("u8", 10, 16, 0.5, 2.0, 9, 9),           # 6  wide stack, chip-kernel layer, power-of-two weight
    ("u8", 10, 8, 2.0, 1.0, 12, 9),           # 7  deliberately too small: the outer cells get no count
    ("u8", 25, 3, 1.37, 0.7, 6, 24),          # 8  fractional on both axes, two K chunks
    ("u8", 57, 2, 64.0, 1.0, 47, 56),         # 9  only cells near the centre land inside
    ("u8", 7, 10, 1.0 / 64, 1.0, 1, 5),       # 10 every stack cell within +-1 layer cell of the centre
    ("dn12", 10, 6, 2.0, 1.0, 13, 9),         # 11
    ("dn12", 16, 8, 2.5, 0.3, 21, 15),        # 12
    ("ddx", 45, 4, 1.5, 1.0, 7, 44),          # 13
    ("dn12", 80, 10, 2.5, 1.0, 27, 60),       # 14 largest chip at its largest radius
)
# one more than the table asks for: one-tap, two-tap, four-tap and outside cells in ONE layer (scale 2.5: integer taps at even shift +
# cell, half taps at odd; a layer radius below stack_layer_radius(8, 2.5) = 21)
ALL_KINDS_CASE = ("u8", 10, 8, 2.5, 1.0, 12, 9)
ORACLE_CASES = (CASES[1], CASES[2], CASES[10])
# at the six chip sizes, within wide_max_radius: also stack_add_scaled's bytes
SIX_CASES = (CASES[2], CASES[3], CASES[4], CASES[11], ("u8", 16, 15, 2.0, 1.0, 31, 15), ("dn12", 16, 8, 2.0, 0.3, 18, 15))
# Which kinds of cell each scale can produce at all (p = s (shift + su) - rint(s shift) per axis): an integer scale gives integer p, one
# tap everywhere; 0.5, 1.5 and 2.5 give integers and halves; 1.37 gives an integer only where shift + su == 0 (the shifts are small: it occurs) and 1/64 where 64 divides shift + su (the shifts
# are near 64 and 128: it occurs), so both show all three.  "outside" needs a
# layer radius below stack_layer_radius(R, s).  kinds: 1 = one tap, 2 = two taps on one axis only, 4 = four taps, 0 = outside the layer
# (case 5 is one below it and still has none: at scale 0.5 the outermost cell lands on 16.5, or on an integer where the shift is odd)
KINDS = {1: (1,), 2: (1,), 3: (1, 2, 4), 4: (1,), 5: (1, 2, 4), 6: (1, 2, 4), 7: (1, 0), 8: (1, 2, 4), 9: (1, 0), 10: (1, 2, 4), 11: (1,),
         12: (1, 2, 4), 13: (1, 2, 4), 14: (1, 2, 4)}

PATTERN_U = (0, 1, -1, 2, -3, 3, -2, 1)
PATTERN_V = (0, -1, 1, -2, 3, -3, 2, -1)


def case_id(case):
    return "-".join(str(round(x, 4)) if isinstance(x, float) else str(x) for x in case[:6])


def base_kind(kind):
    return "dn12" if kind == "dn12" else "u8"


def second_layer(case):
    """the swapped layer's (scale, weight, layer R): half the scale (double it at the smallest), another weight, the radius that scale
    wants but no more than the first layer's, which the pair was sized for"""
    kind, ocw, R, scale, weight, layer_r, _ = case
    s2 = scale / 2 if scale / 2 >= 1.0 / 32 else scale * 2
    return s2, (1.5 if weight == 1.0 else 1.0), min(layer_radius(R, s2), layer_r)


def layers_of(case):
    """the three layers (ocw, swap, scale, weight, layer R): raw, swapped, another chip size"""
    kind, ocw, R, scale, weight, layer_r, ocw2 = case
    return ((ocw, False, scale, weight, layer_r), (ocw, True) + second_layer(case), (ocw2, False, scale, weight, layer_r))


def stack_shift(prior, scale):
    """The stack's shift int32[n][2]: per component the integer nearest prior / scale plus the fixed pattern, where the layer shift then
    stays within 6 px of the pair's prior shift; without the pattern elsewhere (scale 64: any non-zero shift is 64 px away)"""
    prior = np.asarray(prior, np.int64)
    n = prior.shape[0]
    pat = np.stack([np.resize(PATTERN_U, n), np.roll(np.resize(PATTERN_V, n), 3)], axis=1)
    base = np.rint(prior / np.float64(scale)).astype(np.int64)
    near = np.abs(layer_shift(base + pat, scale).astype(np.int64) - prior) <= 6
    return np.ascontiguousarray(np.where(near, base + pat, base), np.int32)


@functools.lru_cache(maxsize=4)
def fixture(case, nulls="placed"):
    """-> dict(c, i0, i1, xy, off, shift (the STACK's), lsh (the first layer's), ocw, R (the stack's), layer_R, scale, weight, kind).
    nulls as stack_fused_common.fixture: "placed", "all" (every point holds a null), "refused" (every chip is all null)"""
    kind, ocw, R, scale, weight, layer_r, _ = case
    c, b0, b1, prior = sf._base(ocw, layer_r)
    i0, i1 = (b0.copy(), b1.copy()) if base_kind(kind) == "u8" else (np.array(spread12(b0), np.float32), np.array(spread12(b1), np.float32))
    shift = stack_shift(prior, scale)
    lsh = layer_shift(shift, scale)
    u, v, cu, cv = fu.geometry(c, lsh, False)
    h = ocw + layer_r
    if nulls == "placed":                                               # (stack_fused_common.fixture's recipe, around the layer's box)
        g = sf.BOX_ONLY[0]; i1[cv[g] + h, cu[g] - 3] = 0
        g = sf.BOX_ONLY[1]; i1[cv[g] + 2, cu[g] + h] = 0
        g = sf.CHIP_ONLY[0]; i0[v[g] - ocw, u[g]] = 0
        g = sf.CHIP_ONLY[1]; i0[v[g] + ocw, u[g] + ocw] = 0
        g = sf.BOTH[0]; i0[v[g], u[g] - 1] = 0; i1[cv[g] + 1, cu[g]] = 0
        g = sf.BOTH[1]; i0[v[g] - 1, u[g] - ocw] = 0; i1[cv[g] - h, cu[g] + 1] = 0
        g = sf.REFUSED; i0[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1] = 0
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
             off=np.ascontiguousarray(c.offset, np.int32), shift=shift, lsh=lsh, ocw=ocw, R=R, layer_R=layer_r, scale=scale, weight=weight,
             kind=kind, what=f"{kind} ocw {ocw} R {R} scale {scale:g} weight {weight:g} layer R {layer_r} nulls {nulls}")
    for a in (f["i0"], f["i1"], f["xy"], f["off"], shift, lsh):
        a.setflags(write=False)
    return f


def layer_view(f):
    """the fixture as its first layer's search sees it: what stack_fused_common.qualifies and kinds count from"""
    return dict(f, shift=f["lsh"], R=f["layer_R"])


def cell_kinds(shift, R, scale, layer_r):
    """Per stack cell of every point, from stack_scaled_axis in numpy -> int[n][S][S]: 0 = a tap that is read lies outside the layer,
    else the taps it reads (1, 2, 4)"""
    shift = np.asarray(shift, np.int32)
    lsh = layer_shift(shift, scale)
    Sl = 2 * layer_r + 1
    au, ju = axis_taps(shift[:, 0], lsh[:, 0], R, layer_r, scale)
    av, jv = axis_taps(shift[:, 1], lsh[:, 1], R, layer_r, scale)
    au, ju, av, jv = au[:, :, None], ju[:, :, None], av[:, None, :], jv[:, None, :]
    two_u, two_v = au != 0, av != 0
    read = (ju >= 0) & (jv >= 0) & (ju + two_u < Sl) & (jv + two_v < Sl)
    return np.where(read, (1 + two_u) * (1 + two_v), 0)


def resample_value(surf, layer_r, shift, R, scale):
    """the definition's value of every stack cell, NaN where a tap that is read lies outside the layer"""
    from stack_scaled_common import resample
    return resample(np.asarray(surf, np.float32), layer_r, shift, R, scale)[0]


def oracle_layers(f, case):
    """the CPU oracle's (record, surfaces, scale, weight, layer R) of the three layers, each searched around its own layer shift"""
    out = []
    for ocw, swap, s, w, rl in layers_of(case):
        rec, _, surf, _ = full_any(f["i0"], f["i1"], f["xy"], f["off"], ocw, rl, 0, shift=layer_shift(f["shift"], s), swap=swap)
        out.append((rec, surf, s, w, rl))
    return out


def oracle_stack(f, case):
    ref = NumpyScaledStack(f["c"].n, f["R"], f["shift"])
    for rec, surf, s, w, rl in oracle_layers(f, case):
        ref.add_scaled(surf, rl, s, w, refused_of(rec))
    return ref


class FusedOrderScaledStack(NumpyScaledStack):
    """NumpyScaledStack fed in the fused order: point by point -- one workgroup finishes a point's layer -- each layer in add order"""

    def add_points(self, layers):
        """layers: [(surf, layer R, scale, weight, refused)] in add order"""
        from stack_scaled_common import resample
        weighted_from = next((i for i, l in enumerate(layers) if l[3] != 1.0), None)
        values = [resample(np.asarray(surf, np.float32), rl, self.shift, self.radius, s)[0] for surf, rl, s, w, _ in layers]
        for g in range(self.n):
            wsum = None
            for i, (surf, rl, s, w, refused) in enumerate(layers):
                if i == weighted_from:
                    wsum = self.cnt[g].astype(np.float64)
                fin = np.isfinite(values[i][g])
                self.sum[g, fin] += np.float64(w) * values[i][g, fin]
                self.cnt[g, fin] += 1
                if wsum is not None:
                    wsum[fin] += np.float64(w)
                if not refused[g]:
                    self.lay[g] += 1
            if wsum is not None:
                if self.wsum is None:
                    self.wsum = np.zeros((self.n, self.cells), np.float64)
                self.wsum[g] = wsum
        self.layers += len(layers)
        return self
