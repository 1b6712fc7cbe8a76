"""No device: the fixtures and the case table of tests/test_stack_scaled_fused.py qualify, from the pixels and from the definition's own
arithmetic (stack_scaled_axis restated in numpy, tests/stack_scaled_common.py).

The four kinds of stack cell -- one tap, two taps on one axis only, four taps, a tap outside the layer -- cannot all occur in every
case of the table: an integer scale (cases 1, 2, 4, 7, 9, 11) gives integer positions, one tap everywhere, and a layer radius of
stack_layer_radius(R, s) or more (most cases) leaves no cell outside.  So every case is checked against the kinds its scale and radii
admit by that reasoning (stack_scaled_fused_common.KINDS), the table as a whole must show all four, and ALL_KINDS_CASE, one case beyond
the table, shows all four in one layer."""
import numpy as np
import pytest

import stack_fused_common as sf
import stack_scaled_fused_common as sc
from stack_scaled_common import NumpyScaledStack, layer_radius, layer_shift

ALL_CASES = sc.CASES + (sc.ALL_KINDS_CASE,)


@pytest.mark.parametrize("case", ALL_CASES + sc.SIX_CASES[4:], ids=sc.case_id)
@pytest.mark.parametrize("nulls", ("placed", "all", "refused"))
def test_fixtures_qualify(case, nulls):
    f = sc.fixture(case, nulls)
    v = sc.layer_view(f)
    nc, nb, ref = sf.kinds(v)
    assert f["c"].n == 24 and np.array_equal(f["lsh"], layer_shift(f["shift"], f["scale"]))
    H, W = f["i0"].shape
    u, w_, cu, cv = sc.fu.geometry(f["c"], f["lsh"], False)
    h = f["ocw"] + f["layer_R"]
    assert (cu - h >= 0).all() and (cu + h < W).all() and (cv - h >= 0).all() and (cv + h < H).all(), "a layer box leaves the image"
    if nulls == "placed":
        assert sf.qualifies(v), f["what"]
        assert ref[sf.REFUSED] and ref.sum() == 1
        assert all(nc[g] == 0 and nb[g] > 0 for g in sf.BOX_ONLY) and all(nc[g] > 0 and nb[g] == 0 for g in sf.CHIP_ONLY)
        assert all(nc[g] > 0 and nb[g] > 0 for g in sf.BOTH)
        assert ((nc == 0) & (nb == 0)).sum() == 17
    elif nulls == "all":
        assert (nb > 0).all() and not ref.any()
    else:
        assert ref.all()


@pytest.mark.parametrize("k", range(len(sc.CASES)))
def test_cells_of_every_case(k):
    kind, ocw, R, scale, weight, layer_r, _ = case = sc.CASES[k]
    f = sc.fixture(case)
    kinds = sc.cell_kinds(f["shift"], R, scale, layer_r)
    counts = {t: int((kinds == t).sum()) for t in (1, 2, 4, 0)}
    print(f"case {k + 1} {f['what']}: one tap {counts[1]}, two taps {counts[2]}, four taps {counts[4]}, outside {counts[0]}")
    present = tuple(t for t in (1, 2, 4, 0) if counts[t])
    assert set(present) == set(sc.KINDS[k + 1]), f"case {k + 1}: kinds {present}, expected {sc.KINDS[k + 1]}"
    if layer_r >= layer_radius(R, scale):
        assert counts[0] == 0                                            # (the promise of mimc3_stack_layer_radius)
    assert counts[0] < kinds.size                                        # some cell lands inside


def test_the_table_shows_every_kind_and_one_case_shows_all():
    seen = set()
    for case in sc.CASES:
        seen |= set(np.unique(sc.cell_kinds(sc.fixture(case)["shift"], case[2], case[3], case[5])).tolist())
    assert seen == {0, 1, 2, 4}
    kind, ocw, R, scale, weight, layer_r, _ = sc.ALL_KINDS_CASE
    kinds = sc.cell_kinds(sc.fixture(sc.ALL_KINDS_CASE)["shift"], R, scale, layer_r)
    assert all((kinds == t).sum() >= 24 for t in (0, 1, 2, 4))
    # case 9 (scale 64): only cells near the centre land inside; case 10 (1/64): every cell within +-1 layer cell of the centre
    k9 = sc.cell_kinds(sc.fixture(sc.CASES[8])["shift"], 2, 64.0, 47)
    assert (k9[:, 2, 2] == 1).all() and (k9[:, 0, :] == 0).all() and (k9[:, :, 4] == 0).all()
    k10 = sc.cell_kinds(sc.fixture(sc.CASES[9])["shift"], 10, 1.0 / 64, 1)
    assert (k10 > 0).all()


def test_the_shift_has_odd_and_negative_components_and_ties_both_ways():
    for case in (sc.CASES[2], sc.CASES[4], sc.CASES[5], sc.CASES[11], sc.CASES[13], sc.ALL_KINDS_CASE):
        s = case[3]
        assert s in (0.5, 2.5)
        sh = sc.fixture(case)["shift"].astype(np.int64)
        assert (sh % 2 != 0).any() and (sh < 0).any() and ((sh < 0) & (sh % 2 != 0)).any()
        p = s * sh.astype(np.float64)
        tie = p - np.floor(p) == 0.5
        lsh = layer_shift(sh, s)
        assert (tie & (lsh < p)).any() and (tie & (lsh > p)).any(), f"scale {s}: ties of rint that round down and that round up"
        assert (lsh[tie] % 2 == 0).all()                                 # half to even


def test_layer_radius_arithmetic_of_the_table():
    from mimc3_amd import api
    want = {1: 4, 2: 9, 3: 19, 4: 46, 5: 18, 6: 9, 7: 17, 8: 5, 9: 129, 10: 1, 11: 13, 12: 21, 13: 7, 14: 26}
    for k, case in enumerate(sc.CASES):
        kind, ocw, R, scale, weight, layer_r, ocw2 = case
        assert layer_radius(R, scale) == want[k + 1], k + 1
        assert 1 <= layer_r <= sf.max_radius(kind, ocw, api), k + 1        # (the library's existing host-side queries)
        assert 1 <= ocw2 <= 80 and ocw2 != ocw
        s2, w2, r2 = sc.second_layer(case)
        assert 1.0 / 64 <= s2 <= 64 and s2 != scale and w2 != weight and 1 <= r2 <= layer_r
    # too small on purpose: 5 (17 < 18), 7 (12 < 17), 9 (47 < 129); one above what the scale wants: 8 (6 > 5), 14 (27 > 26)
    assert [k + 1 for k, c in enumerate(sc.CASES) if c[5] < layer_radius(c[2], c[3])] == [5, 7, 9]


@pytest.mark.parametrize("case", (sc.CASES[1], sc.CASES[2], sc.CASES[7], sc.ALL_KINDS_CASE), ids=sc.case_id)
def test_point_by_point_is_layer_by_layer(case):
    """the fused order (a workgroup finishes one point's layer) against the layer scratch's order: a cell takes one add per layer, so the
    bytes are the same -- on crafted surfaces with NaN and Inf cells, the second layer making the stack weighted"""
    kind, ocw, R, scale, weight, layer_r, _ = case
    f = sc.fixture(case)
    n = f["c"].n
    rng = np.random.default_rng(11)
    layers = []
    for ocw_, swap, s, w, rl in sc.layers_of(case):
        surf = rng.uniform(-1, 1, (n, (2 * rl + 1) ** 2)).astype(np.float32)
        surf[rng.uniform(size=surf.shape) < 0.05] = np.nan
        surf[3, 5] = np.inf
        layers.append((surf, rl, s, w, rng.uniform(size=n) < 0.2))
    a = NumpyScaledStack(n, R, f["shift"])
    for surf, rl, s, w, refused in layers:
        a.add_scaled(surf, rl, s, w, refused)
    b = sc.FusedOrderScaledStack(n, R, f["shift"]).add_points(layers)
    assert a.weighted and b.weighted and a.layers == b.layers == 3
    for x, y in ((a.sum, b.sum), (a.cnt, b.cnt), (a.lay, b.lay), (a.wsum, b.wsum)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert (a.cnt > 0).any() and (a.cnt == 3).any()
