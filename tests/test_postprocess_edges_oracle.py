"""CPU: the inputs of postprocess_edge_common.py on the oracle -- that each input has the property it was built for
(asserted on the oracle's own result), that the oracle agrees with independent plain statements of the decision rules,
and that it equals the compiled reference wherever the reference is defined.  test_postprocess_edges.py then holds the
HIP kernels to the oracle on the same inputs, bit for bit."""
import numpy as np
import pytest

import postprocess_edge_common as pe
from conftest import assert_bits_equal

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- QM
@pytest.fixture(scope="module")
def long_cases():
    return pe.qm_long_cases()


@pytest.mark.parametrize("name", sorted(pe.qm_long_cases()))
def test_qm_long_runs(oracle, reference, long_cases, name):
    a = long_cases[name].arrays()
    d, x, y, st = oracle.qm(*a)
    pe.assert_long_run(name, st)
    assert (d != a[0]).sum() >= 40
    rd, rx, ry, _ = reference.qm(*a)                 # the reference's own loop bound (101 sweeps) is not reached
    assert st[0] < 101
    assert np.array_equal(d, rd)
    assert_bits_equal(x, rx, "dx"); assert_bits_equal(y, ry, "dy")
    for cap in (32, 33, 40):
        cd, cx, cy, cst = oracle.qm(*a, max_sweeps=cap)
        assert cst[0] == min(cap, st[0]) and cst[3] == (oracle.QM_STOP_CAP if cap < st[0] else st[3]), cst.tolist()
        if cap >= st[0]:
            assert np.array_equal(cd, d)
        elif cap < st[0] - 1:
            assert (cd != d).any()                   # the front had not reached the end of the chain
    cst = oracle.qm(*a, max_sweeps=2)[3]
    assert cst[0] == 2 and cst[3] == oracle.QM_STOP_CAP


def test_qm_stats_of_the_older_inputs(oracle):
    """The stop cause on inputs the suite already had: noise ends because nothing changes or by fluctuation, early."""
    from mimc3_amd import synth
    xy = synth.make_grid(48, 40, 60, 60, 20, 20, 1806.0, angle_deg=20.0)
    mvn, nclus, dpf, dx, dy = synth.synth_qm_state(48, 40, seed=3)
    st = oracle.qm(dpf, dx, dy, pe.disc_ruv(5.0), mvn, nclus, xy)[3]
    assert 0 <= st[0] <= 8 and st[3] in (oracle.QM_STOP_UNCHANGED, oracle.QM_STOP_FLUCTUATION)
    assert (st[3] == oracle.QM_STOP_FLUCTUATION) == (st[5] >= 0)
    *_, fit = oracle.qm(dpf, dx, dy, pe.disc_ruv(5.0), mvn, nclus, xy, fit=True)
    assert np.isfinite(fit).any()


def test_qm_leverage_predicts_the_oracle_fit(oracle):
    """qm_leverage (numpy) against the oracle's fit output: one masked point on constant ground, offset by 1 px."""
    c = pe.QmCase("one", 9, 9, pe.disc_ruv(2.0), pe.const_grid(9, 9, 1806.0, 0.0))
    c.set_point(4, 4, [(F32(5.0), F32(-4.0)), (F32(9.0), F32(-4.0))], 0)
    *_, fit = oracle.qm(*c.arrays(), fit=True)
    alpha = pe.qm_leverage(c.ruv, 1806.0, 0.0)[(0, 0)]
    assert abs(fit[4, 4, 0] - (4.0 + alpha)) < 1e-9 and abs(fit[4, 4, 1] + 4.0) < 1e-9
    assert np.isnan(fit[0, 0]).all()


def test_qm_t7(oracle):
    a, zero, empty = pe.qm_t7_case()
    d, x, y, st = oracle.qm(*a)
    assert st[2] > 0 and st[0] >= 2
    masked = (a[4].reshape(a[0].shape + a[4].shape[1:])[..., 0, 4] < 0.6) | (a[0] > 0)
    assert (zero & masked).sum() > 20
    for m in (zero, empty):                                   # T7: left as they were
        assert np.array_equal(d[m], a[0][m])
        assert_bits_equal(x[m], a[1][m]); assert_bits_equal(y[m], a[2][m])
    assert (d != a[0]).sum() > 0


def test_qm_ties(oracle):
    c, pts = pe.qm_tie_case()
    a = c.arrays()
    d, x, y, st = oracle.qm(*a)
    u, v = pts["dup_far"]
    assert a[0][v, u] == 2 and d[v, u] == 0
    u, v = pts["dup_current"]
    assert d[v, u] == 1
    moved = stayed = 0
    for name, (u, v) in pts.items():
        if not name.startswith("near_"):
            continue
        g = v * c.dimx + u
        gap = float(c.mvn[g, 1, 0]) - float(c.mvn[g, 0, 0])
        want = 1 if gap * gap < 0.0001 else 0                 # :2190 in f64 on the f32 means
        assert d[v, u] == want, f"{name}: gap {gap!r}"
        moved += want == 0; stayed += want == 1
    assert moved >= 3 and stayed >= 3


# ---------------------------------------------------------------------------------------------------------- clustering
@pytest.fixture(scope="module")
def pairs():
    return pe.threshold_pairs()


def test_threshold_classes(pairs):
    q = F32(0.25)
    for name in pe.THRESHOLD_CLASSES:
        x, y = pairs[name]
        assert len(x) >= 64 and (x != 0).all() and (y != 0).all(), name
    x, y = pairs["written_lt_fused_ge"]
    assert (pe.written_f32(x, y) < q).all() and (pe.fused_f32(x, y) >= q).all()
    x, y = pairs["written_ge_fused_lt"]
    assert (pe.written_f32(x, y) >= q).all() and (pe.fused_f32(x, y) < q).all()
    x, y = pairs["written_eq"]
    assert (pe.written_f32(x, y) == q).all()
    x, y = pairs["written_vs_f64"]
    assert ((pe.written_f32(x, y) < q) != (pe.exact_f64(x, y) < 0.25)).all()


def test_threshold_pairs_cluster_as_written(oracle, reference, pairs):
    dp, ddx, ddy, others = pe.threshold_candidates(pairs)
    mvn, nclus = oracle.cluster_candidates(dp, kmax=64)
    want = others + np.where(pe.written_f32(ddx, ddy) < F32(0.25), 1, 2)
    assert np.array_equal(nclus, want), np.nonzero(nclus != want)[0][:10]
    assert 0 < (want - others == 1).sum() < len(want)
    rm, rn = reference.cluster_candidates(dp, kmax=64)
    assert np.array_equal(nclus, rn)
    assert_bits_equal(mvn, rm, "mvn")


@pytest.mark.parametrize("ndp", pe.WAVE_NDP)
def test_wave_shapes_vs_reference(oracle, reference, ndp):
    for n in pe.WAVE_N:
        dp = pe.wave_candidates(ndp, n, 0)
        for kmax in (ndp, ndp + 3, 70):
            mvn, nclus = oracle.cluster_candidates(dp, kmax=kmax)
            rm, rn = reference.cluster_candidates(dp, kmax=kmax)
            assert np.array_equal(nclus, rn)
            assert_bits_equal(mvn, rm, f"mvn ndp={ndp} n={n} kmax={kmax}")


def test_shaped_components(oracle, reference):
    names, dp = pe.shaped_components()
    mvn, nclus = oracle.cluster_candidates(dp, kmax=64)
    got = dict(zip(names, nclus.tolist()))
    assert got["singletons_64"] == 64 and got["chain_63_rounds"] == 1 and got["two_interleaved_chains"] == 2
    assert got["bridge_31_32"] == 1 and got["no_bridge_31_32"] == 2 and got["none_valid"] == 0
    assert got["ncc_at_gate"] == 3 and got["only_lane_63"] == 1 and got["squares_overflow"] == 4
    i = names.index("two_interleaved_chains")
    assert mvn[i, 0, 0] < 50 < mvn[i, 1, 0]                  # ids by first member
    i = names.index("two_interleaved_second_first")
    assert mvn[i, 0, 0] > 50 > mvn[i, 1, 0]
    i = names.index("ncc_at_gate")
    assert mvn[i, :3, 4].sum() == F32(32) / F32(64)           # the 32 lanes at exactly 0.1f were dropped, its successor kept
    rm, rn = reference.cluster_candidates(dp, kmax=64)
    assert np.array_equal(nclus, rn)
    assert_bits_equal(mvn, rm, "mvn")


def test_nonfinite_components_follow_the_definition(oracle):
    """Not compared with the compiled reference: a candidate with a NaN or infinite coordinate never labels itself there
    and its sums are then indexed at -1.  The definition: it takes an id and carries nothing."""
    names, dp = pe.nonfinite_components()
    mvn, nclus = oracle.cluster_candidates(dp, kmax=64)
    for i, name in enumerate(names):
        bad = ~np.isfinite(dp[:, i, 0]) | ~np.isfinite(dp[:, i, 1])
        if bad.all():
            assert nclus[i] == 0, name                        # ids taken, none carried: the highest carried id is 0
        carried = mvn[i, :, 4].sum() * 64
        assert carried == (~bad).sum(), name


def test_cancellation_statistics(oracle, reference):
    dp = pe.cancellation_candidates()
    mvn, nclus = oracle.cluster_candidates(dp, kmax=64)
    assert (nclus >= 1).all()
    var = mvn[:, 0, 2:4]
    assert (var < 0).sum() > 50 and (var == 0).sum() > 50     # negative variances and total loss both occur
    rm, rn = reference.cluster_candidates(dp, kmax=64)
    assert np.array_equal(nclus, rn)
    assert_bits_equal(mvn, rm, "mvn")


# ---------------------------------------------------------------------------------------------------------- dpf0
@pytest.mark.parametrize("ndp", pe.WAVE_NDP + (5, 10))
def test_dpf0_fractions(oracle, reference, ndp):
    chosen = 0
    for ratio, mvn, nclus, want in pe.dpf0_fraction_case(ndp):
        n = len(nclus)
        got = oracle.get_dpf0(mvn, nclus, n, 1, ratio).reshape(-1)
        assert np.array_equal(got, want), (ndp, ratio)
        assert want[0] == -1 and want[1] == -1 and (want[2] == 0 or ratio == 1.0)
        assert np.array_equal(reference.get_dpf0(mvn, nclus, n, 1, ratio).reshape(-1), want)
        chosen += (want >= 0).sum()
    assert chosen > 0


def test_dpf0_three_fifths_against_python_0_6(oracle):
    """3/5 and 6/10 in f32 are the f32 nearest to 0.6; the ratio crosses the ABI as f32: equal, so not chosen."""
    mvn = np.zeros((3, 1, 5), F32)
    mvn[0, 0, 4] = F32(3) / F32(5); mvn[1, 0, 4] = F32(6) / F32(10); mvn[2, 0, 4] = np.nextafter(F32(0.6), F32(1))
    got = oracle.get_dpf0(mvn, np.ones(3, np.int32), 3, 1, 0.6).reshape(-1)
    assert got.tolist() == [-1, -1, 0]


# ---------------------------------------------------------------------------------------------------------- dpf1
def test_dpf1_cases(oracle, reference):
    seen = set()
    for name, d0, ruv, mvn, nclus, xy, ref_defined in pe.dpf1_cases(oracle):
        d, x, y, sweeps = oracle.get_dpf1(d0, ruv, mvn, nclus, xy, 16.0, 15.0, sweeps=True)
        d2, x2, y2 = oracle.get_dpf1(d0, ruv, mvn, nclus, xy, 16.0, 15.0)
        assert np.array_equal(d, d2)
        nn = len(ruv)
        if nn - 1 < 3:
            assert sweeps == 0, name
        elif name == "never_filled_island":
            assert sweeps >= nn - 3, name                      # every level down to thres_num = 3 ran
            assert (d[pe.ISLAND] == 0).all() and (d0[pe.ISLAND] == -1).all()
            assert_bits_equal(x[pe.ISLAND].reshape(-1), mvn.reshape(d0.shape + mvn.shape[1:])[pe.ISLAND][..., 0, 0].reshape(-1))
        else:
            assert sweeps >= 1, name
        open_pts = (d0.reshape(-1) < 0) & (nclus > 0)
        assert (d.reshape(-1)[open_pts] >= 0).all(), name
        if name.startswith("zero_apriori"):
            target, neighbour = pe.dpf1_zero_apriori_guards(d0, ruv, nclus, xy)
            assert target.sum() > 0 and neighbour.sum() > 0, name
            # a zero a-priori target is never interpolated: its value is NaN at the snap and the id stays 0
            assert (d[target] == 0).all(), name
            assert_bits_equal(x[target], mvn.reshape(d0.shape + mvn.shape[1:])[target][:, 0, 0], name + " snap")
        if name == "duplicate_rows":
            dup = open_pts & (nclus >= 2) & (mvn[:, 0] == mvn[:, 1]).all(1)
            assert dup.sum() > 100 and (d.reshape(-1)[dup] != 1).all()                # row 1 repeats row 0: never taken
        if ref_defined:
            rd, rx, ry = reference.get_dpf1(d0, ruv, mvn, nclus, xy, 16.0, 15.0)
            assert np.array_equal(d, rd), name
            assert_bits_equal(x, rx, name); assert_bits_equal(y, ry, name)
        seen.add(name)
    assert {"zero_apriori_patch", "zero_apriori_singles", "nn_3", "thin_1x40", "thin_3x3"} <= seen


# ---------------------------------------------------------------------------------------------------------- chain
def test_chain_input_reaches_its_edges(oracle):
    dp, xy, dimx, dimy, mps = pe.chain_case()
    want, d0, st = pe.oracle_chain(oracle, dp, xy, dimx, dimy, mps)
    mvn, nclus = oracle.cluster_candidates(dp, kmax=dp.shape[0])
    at_ratio = (mvn[:, :, 4] == F32(0.6)).any(1)
    assert at_ratio.sum() >= 25 and (d0.reshape(-1)[at_ratio] == -1).all()       # 24 / 40 is not > 0.6f
    assert st[2] > 0                                                             # T7 points in the zero patch
    assert np.isfinite(want[0]).sum() > 0.8 * dimx * dimy
