"""GPU: cluster_kernel, dpf0_kernel, the dpf1 kernels and qm_sweep / qm_finish_sweep (through the C ABI) against the
oracle on the inputs of postprocess_edge_common.py -- long QM runs that use mask words 1 and 2 and every stop rule,
the T7 definition, ties by construction, the 0.5 px clustering threshold where single f32 roundings decide, the
wave-shaped edges of the clustering kernel, statistics under cancellation, dpf0 at the ratio, dpf1 with a zero
a-priori and without an interior.  Everything is compared bit for bit; no generated case is left out."""
import numpy as np
import pytest

import postprocess_edge_common as pe
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.fixture(scope="module")
def ctx(api):
    with api.Context(0) as c:
        yield c


def qm_equal(ctx, oracle, a, what, **kw):
    od, ox, oy, st = oracle.qm(*a, **kw)
    d, x, y, sweeps = ctx.get_dpf_pseudosmoothing(*a, **kw)
    print(f"{what} {kw}: oracle stats {st.tolist()} device sweeps {sweeps} differing ids {int((d != od).sum())}")
    assert sweeps == st[0], f"{what}: device {sweeps} sweeps, oracle {st[0]}"
    assert np.array_equal(d, od), what
    assert_bits_equal(x, ox, what + " dx"); assert_bits_equal(y, oy, what + " dy")
    return d, x, y, st


def short_qm_input():
    from mimc3_amd import synth
    xy = synth.make_grid(48, 40, 60, 60, 20, 20, 1806.0, angle_deg=20.0)
    mvn, nclus, dpf, dx, dy = synth.synth_qm_state(48, 40, seed=1, p_out=0.45, p_wrong=0.1)     # 4 sweeps on the oracle
    return dpf, dx, dy, pe.disc_ruv(5.0), mvn, nclus, xy


# ---------------------------------------------------------------------------------------------------------- QM
@pytest.mark.parametrize("name", sorted(pe.qm_long_cases()))
def test_qm_long_runs(ctx, oracle, name):
    a = pe.qm_long_cases()[name].arrays()
    st = oracle.qm(*a)[3]
    pe.assert_long_run(name, st)
    qm_equal(ctx, oracle, a, name)
    for cap in (32, 33, 40, 2, 64, 65):
        cst = qm_equal(ctx, oracle, a, name, max_sweeps=cap)[3]
        if cap < st[0]:
            assert cst[3] == oracle.QM_STOP_CAP and cst[0] == cap
    # the same context, a short input: nothing of the long run may be left in the flags, slots or the stack
    s = short_qm_input()
    qm_equal(ctx, oracle, s, name + " then short")


def test_qm_max_sweeps_bounds(api, ctx, oracle):
    s = short_qm_input()
    st = qm_equal(ctx, oracle, s, "short, 255 sweeps allowed", max_sweeps=255)[3]
    assert 2 <= st[0] < 32
    with pytest.raises(api.Mimc3Error):
        ctx.get_dpf_pseudosmoothing(*s, max_sweeps=256)
    qm_equal(ctx, oracle, s, "short after the refusal")
    a = pe.qm_long_cases()["fluct_97_3blocks"].arrays()
    st = qm_equal(ctx, oracle, a, "97-point chain, 255 sweeps allowed", max_sweeps=255)[3]
    assert st[0] >= 65 and st[3] == oracle.QM_STOP_FLUCTUATION


def test_qm_t7(ctx, oracle):
    a, zero, empty = pe.qm_t7_case()
    assert oracle.qm(*a)[3][2] > 0
    d, x, y, st = qm_equal(ctx, oracle, a, "t7")
    for m in (zero, empty):
        assert np.array_equal(d[m], a[0][m])
        assert_bits_equal(x[m], a[1][m]); assert_bits_equal(y[m], a[2][m])
    qm_equal(ctx, oracle, a, "t7", max_sweeps=1)


def test_qm_ties(ctx, oracle):
    c, pts = pe.qm_tie_case()
    a = c.arrays()
    d, x, y, st = qm_equal(ctx, oracle, a, "ties")
    u, v = pts["dup_far"]
    assert d[v, u] == 0
    u, v = pts["dup_current"]
    assert d[v, u] == 1


# ---------------------------------------------------------------------------------------------------------- clustering
def cluster_equal(ctx, oracle, dp, kmax, what):
    rm, rn = oracle.cluster_candidates(dp, kmax=kmax)
    mvn, nclus = ctx.calc_mean_var_num_dp_cluster(dp, kmax)
    assert np.array_equal(nclus, rn), f"{what}: nclus differs at {np.nonzero(nclus != rn)[0][:10].tolist()}"
    assert_bits_equal(mvn, rm, what + " mvn")
    return mvn, nclus


def test_threshold_pairs(ctx, oracle):
    pairs = pe.threshold_pairs()
    for name in pe.THRESHOLD_CLASSES:
        assert len(pairs[name][0]) >= 64
    dp, ddx, ddy, others = pe.threshold_candidates(pairs)
    mvn, nclus = cluster_equal(ctx, oracle, dp, 64, "threshold pairs")
    want = others + np.where(pe.written_f32(ddx, ddy) < F32(0.25), 1, 2)
    assert np.array_equal(nclus, want)


@pytest.mark.parametrize("ndp", pe.WAVE_NDP)
def test_wave_shapes(api, ctx, oracle, ndp):
    for n in pe.WAVE_N:
        dp = pe.wave_candidates(ndp, n, 0)
        need = int(oracle.cluster_candidates(dp, kmax=ndp)[1].max())
        for kmax in sorted({need, ndp, ndp + 3, 65, 70, 133}):
            if kmax >= need and kmax > 0:
                cluster_equal(ctx, oracle, dp, kmax, f"ndp={ndp} n={n} kmax={kmax}")
        if need > 1:
            with pytest.raises(api.Mimc3Error):
                ctx.calc_mean_var_num_dp_cluster(dp, need - 1)
            cluster_equal(ctx, oracle, dp, need, f"ndp={ndp} n={n} after the capacity error")


def test_ndp_65_is_refused(api, ctx):
    dp = np.zeros((65, 4, 3), F32)
    dp[:, :, 2] = 0.9
    with pytest.raises(api.Mimc3Error):
        ctx.calc_mean_var_num_dp_cluster(dp, 65)
    xy = pe.const_grid(2, 2, 1000.0, 500.0)
    with pytest.raises(api.Mimc3Error):
        ctx.mimc2_postprocess(dp, xy, 2, 2, 16.0, 15.0, 300.0)


def test_shaped_components(ctx, oracle):
    names, dp = pe.shaped_components()
    mvn, nclus = cluster_equal(ctx, oracle, dp, 64, "shapes")
    got = dict(zip(names, nclus.tolist()))
    assert got["singletons_64"] == 64 and got["chain_63_rounds"] == 1 and got["bridge_31_32"] == 1
    cluster_equal(ctx, oracle, dp[:, 1:2], 1, "63-round chain alone, kmax 1")
    cluster_equal(ctx, oracle, dp, 100, "shapes, kmax 100")


def test_nonfinite_components(ctx, oracle):
    """NaN and +-Inf coordinates with a passing ncc: undefined in the reference, defined in DESIGN.md section 2."""
    names, dp = pe.nonfinite_components()
    cluster_equal(ctx, oracle, dp, 64, "non-finite")


def test_cancellation_statistics(ctx, oracle):
    dp = pe.cancellation_candidates()
    mvn, _ = cluster_equal(ctx, oracle, dp, 64, "cancellation")
    assert (mvn[:, 0, 2:4] < 0).sum() > 50


# ---------------------------------------------------------------------------------------------------------- dpf0
@pytest.mark.parametrize("ndp", pe.WAVE_NDP + (5, 10))
def test_dpf0_fractions(ctx, ndp):
    for ratio, mvn, nclus, want in pe.dpf0_fraction_case(ndp):
        got = ctx.get_dpf0(mvn, nclus, len(nclus), 1, ratio).reshape(-1)
        assert np.array_equal(got, want), (ndp, ratio, got.tolist(), want.tolist())


def test_dpf0_three_fifths_against_python_0_6(ctx):
    mvn = np.zeros((3, 1, 5), F32)
    mvn[0, 0, 4] = F32(3) / F32(5); mvn[1, 0, 4] = F32(6) / F32(10); mvn[2, 0, 4] = np.nextafter(F32(0.6), F32(1))
    assert ctx.get_dpf0(mvn, np.ones(3, np.int32), 3, 1, 0.6).reshape(-1).tolist() == [-1, -1, 0]


# ---------------------------------------------------------------------------------------------------------- dpf1
def test_dpf1_cases(ctx, oracle):
    for name, d0, ruv, mvn, nclus, xy, _ in pe.dpf1_cases(oracle):
        rd, rx, ry, rs = oracle.get_dpf1(d0, ruv, mvn, nclus, xy, 16.0, 15.0, sweeps=True)
        if name.startswith("zero_apriori"):
            target, neighbour = pe.dpf1_zero_apriori_guards(d0, ruv, nclus, xy)
            assert target.sum() > 0 and neighbour.sum() > 0 and (rd[target] == 0).all(), name
        d, x, y, sweeps = ctx.get_dpf1(d0, ruv, mvn, nclus, xy, 16.0, 15.0)
        print(f"dpf1 {name}: oracle sweeps {rs} device sweeps {sweeps} differing ids {int((d != rd).sum())}")
        # both count every pass over the grid, the last, empty pass of each level included (the reference's NOI)
        assert sweeps == rs, name
        assert np.array_equal(d, rd), name
        assert_bits_equal(x, rx, name + " dx"); assert_bits_equal(y, ry, name + " dy")


# ---------------------------------------------------------------------------------------------------------- chain
def test_chain(ctx, oracle):
    dp, xy, dimx, dimy, mps = pe.chain_case()
    want, d0, st = pe.oracle_chain(oracle, dp, xy, dimx, dimy, mps)
    assert st[2] > 0
    got = ctx.mimc2_postprocess(dp, xy, dimx, dimy, 16.0, 15.0, mps)
    assert_bits_equal(got.reshape(5, -1), want, "vxyexyqual")
