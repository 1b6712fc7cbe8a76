"""GPU: QM pseudo-smoothing kernels (through the C ABI) against golden vectors and the oracle.
Bar: identical cluster ids, bit-identical dpf_dx/dpf_dy, same sweep count."""
import numpy as np
import pytest

from conftest import assert_bits_equal, golden_files
from mimc3_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.mark.parametrize("path", golden_files("qm_"), ids=lambda p: p.split("/")[-1][:-4])
def test_golden(api, oracle, path):
    z = np.load(path)
    dimy, dimx = z["dpf_in"].shape
    ruv = api.get_ruv_neighbor(z["xyuvav"], dimx, dimy, float(z["meter_per_spacing"]), float(z["radius"]))
    assert np.array_equal(ruv, z["ruv"])
    with api.Context(0) as ctx:
        d, x, y, sweeps = ctx.get_dpf_pseudosmoothing(z["dpf_in"], z["dx_in"], z["dy_in"], ruv, z["mvn"], z["nclus"], z["xyuvav"])
    assert np.array_equal(d, z["dpf_out"])
    assert_bits_equal(x, z["dx_out"], "dx")
    assert_bits_equal(y, z["dy_out"], "dy")
    _, _, _, stats = oracle.qm(z["dpf_in"], z["dx_in"], z["dy_in"], ruv, z["mvn"], z["nclus"], z["xyuvav"])
    assert sweeps == stats[0]


def qm_inputs(dimx, dimy, seed, ang, p_out=0.45):
    """A realistic QM input built without the reference: synthetic candidates, single-linkage
    clustered (<0.5 px) by a small numpy stand-in, most populated cluster as the initial pick.
    Any candidate tensor is a valid QM input; parity is HIP vs oracle on the same tensor."""
    xy = synth.make_grid(dimx, dimy, 60, 60, 20, 20, 1806.0, angle_deg=ang)
    dp = synth.synth_candidates(dimx, dimy, seed=seed, p_out=p_out)
    k, n, _ = dp.shape
    mvn = np.zeros((n, k, 5), np.float32)
    nclus = np.zeros(n, np.int32)
    dpf = -np.ones(n, np.int32)
    dx = np.full(n, np.nan, np.float32)
    dy = np.full(n, np.nan, np.float32)
    for i in range(n):
        pts = dp[:, i, :2].astype(np.float64)
        lab = -np.ones(k, int)
        nl = 0
        for a in range(k):
            if lab[a] >= 0:
                continue
            lab[a] = nl
            todo = [a]
            while todo:
                b = todo.pop()
                near = np.where((lab < 0) & (np.hypot(pts[:, 0] - pts[b, 0], pts[:, 1] - pts[b, 1]) < 0.5))[0]
                lab[near] = nl
                todo.extend(near.tolist())
            nl += 1
        nclus[i] = nl
        for c in range(nl):
            m = pts[lab == c]
            mvn[i, c] = [m[:, 0].mean(), m[:, 1].mean(), m[:, 0].var(), m[:, 1].var(), len(m) / k]
        big = int(np.argmax(mvn[i, :nl, 4]))
        dpf[i] = big
        dx[i] = mvn[i, big, 0]
        dy[i] = mvn[i, big, 1]
    return xy, mvn, nclus, dpf.reshape(dimy, dimx), dx.reshape(dimy, dimx), dy.reshape(dimy, dimx)


@pytest.mark.parametrize("dims", [(48, 40, 3, 20.0, 0.45), (150, 120, 4, -135.0, 0.5), (33, 31, 6, 90.0, 0.6)])
def test_vs_oracle(api, oracle, dims):
    dimx, dimy, seed, ang, p_out = dims
    xy, mvn, nclus, dpf, dx, dy = qm_inputs(dimx, dimy, seed, ang, p_out)
    mps = float(np.float32(xy[1, 0] - xy[0, 0]))
    ruv = api.get_ruv_neighbor(xy, dimx, dimy, mps, 5.0)
    wd, wx, wy, stats = oracle.qm(dpf, dx, dy, ruv, mvn, nclus, xy)
    with api.Context(0) as ctx:
        d, x, y, sweeps = ctx.get_dpf_pseudosmoothing(dpf, dx, dy, ruv, mvn, nclus, xy)
        assert np.array_equal(d, wd) and sweeps == stats[0]
        assert_bits_equal(x, wx)
        assert_bits_equal(y, wy)
        assert (d != dpf).sum() > 0
        # capped sweep count (BASELINE config C5 runs 10): equals the oracle capped at the same count
        d2, x2, y2, s2 = ctx.get_dpf_pseudosmoothing(dpf, dx, dy, ruv, mvn, nclus, xy, max_sweeps=2)
        od, ox, oy, ost = oracle.qm(dpf, dx, dy, ruv, mvn, nclus, xy, max_sweeps=2)
        assert np.array_equal(d2, od) and s2 == ost[0]
        assert_bits_equal(x2, ox)
        assert_bits_equal(y2, oy)


def test_cap_below_a_long_run(api, oracle):
    """max_sweeps=2 on an input whose uncapped run is far longer (39 sweeps): the cap itself decides.  (One of
    test_vs_oracle's inputs stops by itself before sweep 2, so its capped leg does not reach the cap.)"""
    import postprocess_edge_common as pe
    a = pe.qm_domino(200, 5, chain=40).arrays()
    full = oracle.qm(*a)
    od, ox, oy, ost = oracle.qm(*a, max_sweeps=2)
    assert full[3][0] > 2 and ost[0] == 2 and ost[3] == pe.QM_STOP_CAP and (od != full[0]).any()
    with api.Context(0) as ctx:
        d2, x2, y2, s2 = ctx.get_dpf_pseudosmoothing(*a, max_sweeps=2)
    assert np.array_equal(d2, od) and s2 == ost[0]
    assert_bits_equal(x2, ox)
    assert_bits_equal(y2, oy)


def test_nan_and_unassigned_points(api, oracle):
    """dpf == -1 / NaN displacements are skipped as neighbours and never investigated (:2035, :2116)."""
    xy, mvn, nclus, dpf, dx, dy = qm_inputs(40, 36, 9, 60.0)
    rng = np.random.default_rng(3)
    hole = rng.random(dpf.shape) < 0.15
    dpf[hole] = -1
    dx[hole] = np.nan
    dy[hole] = np.nan
    mps = float(np.float32(xy[1, 0] - xy[0, 0]))
    ruv = api.get_ruv_neighbor(xy, 40, 36, mps, 5.0)
    wd, wx, wy, stats = oracle.qm(dpf, dx, dy, ruv, mvn, nclus, xy)
    with api.Context(0) as ctx:
        d, x, y, sweeps = ctx.get_dpf_pseudosmoothing(dpf, dx, dy, ruv, mvn, nclus, xy)
    assert np.array_equal(d, wd) and sweeps == stats[0]
    assert_bits_equal(x, wx)
    assert_bits_equal(y, wy)
    assert (d[hole] == -1).all()
