"""CPU: the fused stack layers (mimc3_stack_add_fused) without a device -- the symbols and their argument counts, the fixtures of the GPU
tests counted from their pixels and qualified on the CPU oracle, the order of the adds (a fused layer adds point by point; the stack is
the one fed whole surfaces), and the radius limits per pixel class restated from the library's existing queries."""
import os
import re

import numpy as np
import pytest

import stack_fused_common as sf
from conftest import ROOT
from stack_common import NumpyStack, refused_of


def test_symbols_and_argument_counts():
    from mimc3_amd import api
    hdr = open(os.path.join(ROOT, "include", "mimc3_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("mimc3_stack_add_fused", 6), ("mimc3_stack_add_fused_dev", 8), ("mimc3_stack_fused_max_radius", 2)):
        fn = getattr(api._lib, name)
        assert len(fn.argtypes) == nargs, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
    for name in ("stack_add_fused", "stack_add_fused_dev", "stack_fused_max_radius"):
        assert callable(getattr(api.Context, name))
    assert api._lib.mimc3_stack_fused_max_radius(None, 16) == 0        # (no context: 0, no error)


def test_every_gpu_fixture_holds_every_kind_of_point():
    cases = [("u8", o, r) for o, r, _ in sf.U8_CASES] + [("dn12", o, r) for o, r, _ in sf.U16_CASES] + [("u8", o, r) for o, r, _ in sf.U16_CASES]
    for kind, ocw, R in sorted(set(cases)):
        f = sf.fixture(ocw, R, kind)
        assert sf.qualifies(f), f["what"]
        nc, nb, ref = sf.kinds(f)
        assert ref[sf.REFUSED] and ref.sum() == 1
        for g in sf.BOX_ONLY:
            assert nc[g] == 0 and nb[g] == 1
        for g in sf.CHIP_ONLY:
            assert nc[g] == 1 and nb[g] == 0
        for g in sf.BOTH:
            assert nc[g] == 1 and nb[g] == 1
    f = sf.fixture(10, 4, "u8", "all")
    nc, nb, ref = sf.kinds(f)
    assert (nb > 0).all() and not ref.any()
    f = sf.fixture(10, 4, "u8", "refused")
    assert sf.kinds(f)[2].all()


@pytest.mark.parametrize("kind,ocw,R,ocw2", sf.ORACLE_CASES)
def test_oracle_qualifies_the_fixture_and_the_order_of_the_adds(kind, ocw, R, ocw2):
    """On the CPU oracle: the refused point has status -3 in every layer and nothing else has in the first, at least 20 points have a
    fit after stacking; and NumpyStack fed in the fused order (point by point) is NumpyStack fed whole surfaces, byte for byte"""
    f = sf.fixture(ocw, R, kind)
    n = f["c"].n
    layers = sf.oracle_layers(f, ocw2)
    rec0 = layers[0][0]
    assert rec0[sf.REFUSED, 2] == -3 and (rec0[:, 2] == -3).sum() == 1
    whole = NumpyStack(n, R, f["shift"])
    for rec, surf in layers:
        whole.add(surf, refused_of(rec))
    fused = sf.FusedOrderStack(n, R, f["shift"]).add_points([(surf, refused_of(rec)) for rec, surf in layers])
    assert fused.layers == whole.layers == 3
    assert fused.sum.tobytes() == whole.sum.tobytes() and np.array_equal(fused.cnt, whole.cnt) and np.array_equal(fused.lay, whole.lay)
    for k, mc in sf.FINISHES:
        sf.same_bytes(fused.finish(k, mc), whole.finish(k, mc), f"{f['what']} npeaks {k} min_count {mc}")
    rec = whole.finish(0, 1)[0]
    assert (rec[:, 2] >= -1).sum() >= 20, f["what"]
    # (the refused point's chip is null in image 0: the swapped layer, whose chip comes from image 1, takes the point, and so does a third
    #  layer with a larger chip -- count tells the layers apart)
    assert 1 <= whole.lay[sf.REFUSED] <= 2 and (np.delete(whole.lay, sf.REFUSED) == 3).all()


def test_radius_limits_restate_the_existing_queries():
    from mimc3_amd import api
    for ocw in range(0, 83):
        assert sf.max_radius("u8", ocw, api) == api.wide_class_max_radius(ocw)
    for ocw in range(1, 81):
        assert sf.max_radius("dn12", ocw, api) == api.wide_planes_max_radius(ocw) >= 27
        other = sf.max_radius("dn16", ocw, api)
        assert other == (api.wide_max_radius(ocw) if ocw in sf.SIX else 15) and other >= 15
    assert sf.max_radius("dn12", 80, api) == 27 and sf.max_radius("dn12", 68, api) == 47
    for o, r, _ in sf.U8_CASES:
        assert r <= sf.max_radius("u8", o, api)
    for o, r, _ in sf.U16_CASES:
        assert r <= sf.max_radius("dn12", o, api)
