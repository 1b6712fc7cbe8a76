"""GPU: the accumulating (ACC) forms of the four run-time-ocw matrix-core searches -- stack_add_fused, stack_acc.h -- at every pixel phase
of chip and window origin with every null class, and with one null at every position that a byte mask, a chunk boundary or a tile-window
edge can get wrong: the fixtures and calls of tests/test_chip_phases.py, whose oracle runs they share.

Every point is finished by exactly one workgroup -- the clean form, or the masked form in flag mode behind it -- which is what lets the
ACC forms add into the stack with plain read-modify-writes.  One stack_add_fused on a fresh stack per call; the path is asserted.  The
judge is chip_phase_common.acc_judge, qualified without a device by tests/test_chip_phases_cpu.py: stack_finish(4, 1) against
stack_common.NumpyStack fed the CPU ORACLE's surface -- the mean surface bit for bit, the layer counts, record and candidates -- and
stack_finish(0, 2), whose surface is all NaN unless some cell was added twice.  No tolerance."""
import pytest

import chip_phase_common as cp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.mark.parametrize("part", cp.ACC_PARTS)
@pytest.mark.parametrize("case", cp.ACC_PHASE_CASES, ids=[cp.case_id(c) for c in cp.ACC_PHASE_CASES])
def test_one_fused_layer_at_every_phase_with_every_null_class(api, case, part):
    """the 64 points of the phase fixture, clean and null points in one launch pair: the four offsets in u with the a-priori shift, and
    the two swapped calls"""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for k in cp.PARTS[part]:
            offset, shift, swap = calls[k]
            o_rec, o_surf = cp.phase_oracle(case, k)
            got = cp.acc_call(ctx, entry, f.xy, radius, offset, ocw, shift, swap)
            cp.acc_judge(got, o_rec, o_surf, radius, shift, f"{cp.case_id(case)}, offset {offset.tolist()}, swap {swap}")


@pytest.mark.parametrize("case", cp.ACC_SWEEP_CASES, ids=[cp.case_id(c) for c in cp.ACC_SWEEP_CASES])
def test_one_fused_layer_with_one_null_per_point(api, case):
    """every point holds one null, so every one is finished by the masked ACC form"""
    entry, kind, ocw, radius = case
    fx = cp.sweep_fixture(case)
    o_rec, o_surf = cp.sweep_oracle(fx)
    with api.Context(0) as ctx:
        ctx.set_images(fx.i0, fx.i1)
        got = cp.acc_call(ctx, entry, fx.xy, radius, fx.offset, ocw, fx.shift, False)
    cp.acc_judge(got, o_rec, o_surf, radius, fx.shift, cp.case_id(case))
    assert (got[0][2] == 1).all()
