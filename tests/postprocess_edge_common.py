"""Inputs that reach the decision edges of the stages behind the matcher -- candidate clustering, dpf0, dpf1 and the QM
pseudo-smoothing -- shared by test_postprocess_edges_oracle.py (CPU: the oracle against independent statements and the
compiled reference) and test_postprocess_edges.py (GPU: the HIP kernels against the oracle, bit for bit).

Every generator is deterministic.  Where a property of an input matters (a QM run of >= 33 sweeps, a class of
threshold pairs with >= 64 members, a T7 count > 0), the tests assert it on the oracle's result before anything is
compared, so a change here cannot make them vacuous.
"""
import numpy as np

F32 = np.float32


QM_STOP_UNCHANGED, QM_STOP_FLUCTUATION, QM_STOP_CAP = 0, 1, 2          # oracle stats[3]


def assert_long_run(name, st):
    """The properties the long QM inputs exist for, by name, on the oracle's stats."""
    want65 = "_70_" in name or "_97_" in name
    assert st[0] >= (65 if want65 else 33), f"{name}: {st[0]} sweeps"
    if name.startswith("fluct"):
        assert st[3] == QM_STOP_FLUCTUATION and st[5] >= 32 and st[4] >= st[5], f"{name}: stats {st.tolist()}"
    else:
        assert st[3] == QM_STOP_UNCHANGED and st[4] == -1, f"{name}: stats {st.tolist()}"


def dpf1_zero_apriori_guards(d0, ruv, nclus, xy):
    """(open points with a zero a-priori, assigned zero-a-priori points within the neighbour list of an open point)."""
    dimy, dimx = d0.shape
    zero = ((xy[:, 4] == 0) & (xy[:, 5] == 0)).reshape(dimy, dimx)
    opn = (d0 < 0) & (nclus.reshape(dimy, dimx) > 0)
    near_open = np.zeros_like(opn)
    for du, dv in ruv.tolist():
        src = opn[max(0, -dv):dimy - max(0, dv), max(0, -du):dimx - max(0, du)]
        near_open[max(0, dv):dimy - max(0, -dv), max(0, du):dimx - max(0, -du)] |= src
    return opn & zero, zero & (d0 >= 0) & near_open


# =====================================================================================================================
# QM: long runs by construction
# =====================================================================================================================
def disc_ruv(radius):
    """Neighbour offsets (du, dv) with du^2 + dv^2 <= radius^2, row-major like get_ruv_neighbor's."""
    k = int(np.floor(radius))
    return np.array([(u, v) for v in range(-k, k + 1) for u in range(-k, k + 1) if u * u + v * v <= radius * radius], np.int32)


def qm_leverage(ruv, vx, vy):
    """How much each neighbour's value moves the QM fit at the centre: the fit (weighted quadratic least squares
    evaluated at the origin, MIMC_module.c:2144-2153, :2314-2409) is linear in the data, fit = sum_k L[k] * z[k], for a
    point whose neighbours are all valid.  Plain f64 numpy -- used to place clusters, never to judge a result."""
    eig0 = 1500.0 / 300.0
    eig1 = eig0 / 3.0
    den = eig0 * eig1 * (vx * vx + vy * vy)
    i0 = (eig1 * vx * vx + eig0 * vy * vy) / den
    i1 = (eig0 - eig1) * vx * vy / den
    i3 = (eig1 * vy * vy + eig0 * vx * vx) / den
    x = ruv[:, 0].astype(np.float64)
    y = ruv[:, 1].astype(np.float64)
    w = np.exp(-(i0 * x * x + 2 * i1 * x * y + i3 * y * y))
    a = np.stack([x * x, x * y, y * y, x, y, np.ones_like(x)], 1)
    lev = np.linalg.solve(a.T @ (a * w[:, None]), (a * w[:, None]).T)[5]
    return {(int(u), int(v)): float(l) for (u, v), l in zip(ruv.tolist(), lev)}


def const_grid(dimx, dimy, vx, vy, spacing=20.0, mpp=15.0):
    """xyuvav [N][6] with a constant a-priori velocity (x fastest)."""
    uu, vv = np.meshgrid(60.0 + spacing * np.arange(dimx), 60.0 + spacing * np.arange(dimy))
    xy = np.stack([uu * mpp, -vv * mpp, uu, vv, np.full_like(uu, vx), np.full_like(uu, vy)], -1).reshape(-1, 6)
    return np.ascontiguousarray(xy, np.float64)


class QmCase:
    """One QM input: everything get_dpf_pseudosmoothing takes."""

    def __init__(self, name, dimx, dimy, ruv, xy, kmax=4, ground=(4.0, -4.0)):
        self.name, self.dimx, self.dimy, self.ruv, self.xy = name, dimx, dimy, ruv, xy
        n = dimx * dimy
        self.mvn = np.zeros((n, kmax, 5), F32)
        self.mvn[:, 0] = (ground[0], ground[1], 0.0, 0.0, 1.0)          # one full cluster: unmasked (fraction >= 0.6)
        self.nclus = np.ones(n, np.int32)
        self.dpf = np.zeros(n, np.int32)
        self.ground = ground

    def set_point(self, u, v, clusters, pick, frac=0.25):
        g = v * self.dimx + u
        self.mvn[g] = 0
        for c, (cu, cv) in enumerate(clusters):
            self.mvn[g, c] = (cu, cv, 0.0, 0.0, frac)
        self.nclus[g] = len(clusters)
        self.dpf[g] = pick

    def arrays(self):
        """(dpf, dx, dy, ruv, mvn, nclus, xyuvav): dx/dy are the picked clusters' means, NaN where dpf < 0."""
        n = self.dimx * self.dimy
        ok = self.dpf >= 0
        pick = np.where(ok, self.dpf, 0)
        dx = np.where(ok, self.mvn[np.arange(n), pick, 0], np.nan).astype(F32)
        dy = np.where(ok, self.mvn[np.arange(n), pick, 1], np.nan).astype(F32)
        shp = (self.dimy, self.dimx)
        return self.dpf.reshape(shp).copy(), dx.reshape(shp), dy.reshape(shp), self.ruv, self.mvn, self.nclus, self.xy


def qm_domino(dimx, dimy, chain, osc=0, along="u", radius=2.0, h=1.0, name=None):
    """A QM input whose run length is set by construction.

    A "domino chain": `chain` adjacent masked points on the middle line of a grid of otherwise unmasked, constant
    points.  Each has two clusters at ground + m -+ h along the line's axis and starts in the lower one.  With L the
    leverages of qm_leverage along the line and S their sum over the line, the fit of a chain point whose predecessors
    have all flipped but one is S*m - (alpha + 2*L1)*h, and S*m - alpha*h once that last predecessor has flipped too;
    m = -(alpha + L1) * h / (1 - S) puts the point's decision boundary half way between the two (margin L1*h), so
    point i flips in sweep i + 1 and not before: one sweep per point.  Point 0's lower cluster lies 2 px further down,
    which makes it flip in sweep 1; `radius` unmasked points in the lower state follow the last chain point, or the far
    end would see the ground there and start a second front towards the first.  The masks of successive sweeps are windows that move along the chain, all
    different, so the run ends when nothing changes any more (chain - 1 sweeps: the last point has no successor to pull it over).

    An "oscillator": `osc` adjacent masked points further along the same line, more than twice the radius away from
    the chain, clusters at ground -+ h_i, starting in alternating states.  With D = diag(s) L diag(s) (s the
    alternating signs) every point flips in every sweep iff D h < 0 for the positive vector h: h is the eigenvector of
    the lowest (negative) eigenvalue of D, scaled to min h_i = 0.25 px.  Its mask is the same after every sweep, so once
    the chain has run out the next mask equals the previous one: a fluctuation stop against a mask of index ~ chain.

    along="u": the line is a row, the a-priori flow points along +u; along="v": a column, flow along +v."""
    ruv = disc_ruv(radius)
    k = int(np.floor(radius))
    vx, vy = (1806.0, 0.0) if along == "u" else (0.0, 1806.0)
    lev = qm_leverage(ruv, vx, vy)
    line = [lev[(j, 0) if along == "u" else (0, j)] for j in range(-k, k + 1)]        # leverages along the line
    alpha, l1, s_sum = line[k], line[k + 1], float(np.sum(line))
    assert l1 > 0 and s_sum < 1
    m = -(alpha + l1) * h / (1.0 - s_sum)
    c = QmCase(name or f"domino_{dimx}x{dimy}_{along}_c{chain}_o{osc}", dimx, dimy, ruv, const_grid(dimx, dimy, vx, vy))
    gx, gy = c.ground
    length, mid = (dimx, dimy // 2) if along == "u" else (dimy, dimx // 2)
    need = k + chain + k + ((2 * k + 1 + osc) if osc else 0) + k
    assert need <= length and mid >= k and (dimy if along == "u" else dimx) - 1 - mid >= k, "line does not fit"

    def put(t, values, pick, frac=0.25):
        u, v = (t, mid) if along == "u" else (mid, t)
        cl = [(gx + a, gy) if along == "u" else (gx, gy + a) for a in values]
        c.set_point(u, v, [(F32(a), F32(b)) for a, b in cl], pick, frac)

    for i in range(chain):
        put(k + i, (m - h - (2.0 if i == 0 else 0.0), m + h), 0)
    for i in range(k):                      # unmasked anchors in the lower state: the far end sees a chain that goes on
        put(k + chain + i, (m - h,), 0, frac=1.0)
    if osc:
        sgn = np.array([1.0 if i % 2 == 0 else -1.0 for i in range(osc)])
        d = np.zeros((osc, osc))
        for i in range(osc):
            for j in range(osc):
                if abs(i - j) <= k:
                    d[i, j] = sgn[i] * sgn[j] * line[k + j - i]
        w, vec = np.linalg.eigh(d)
        hv = vec[:, 0] * np.sign(vec[0, 0])
        assert w[0] < 0 and (hv > 0).all(), "no oscillating solution for this line"
        hv = hv * (0.25 / hv.min())
        t0 = k + chain + k + 2 * k + 1
        for i in range(osc):
            put(t0 + i, (-hv[i], hv[i]), i % 2)
    return c


# (name, builder): the long runs the tests assert on.  One grid of N <= 1024 (a single finish block), and grids of
# several finish blocks with N a multiple of neither 1024 nor 256, the line running down a column so that it crosses
# every block.
def qm_long_cases():
    return {
        "unchanged_40_1block": qm_domino(200, 5, chain=40, along="u"),                    # N = 1000
        "fluct_40_1block": qm_domino(200, 5, chain=40, osc=8, along="u"),
        "unchanged_40_3blocks": qm_domino(13, 211, chain=40, along="v"),                  # N = 2743 = 2*1024 + 695
        "fluct_40_3blocks": qm_domino(13, 211, chain=40, osc=8, along="v"),
        "unchanged_70_3blocks": qm_domino(13, 211, chain=70, along="v"),
        "fluct_70_1block": qm_domino(200, 5, chain=70, osc=8, along="u"),
        "fluct_97_3blocks": qm_domino(13, 211, chain=97, osc=9, along="v"),
    }


def qm_t7_case(dimx=60, dimy=50, seed=21):
    """Zero a-priori velocity (rock): den = 0 in the weights, every weight NaN, the fit NaN, no candidate is nearest --
    the T7 definition leaves such a point as it is and counts it.  A patch, single points, and points with an empty
    cluster list (nclus = 0 with dpf = 0: valid at the ABI, same path) inside the masked region."""
    from mimc3_amd import synth
    xy = synth.make_grid(dimx, dimy, 60, 60, 20, 20, 1806.0, angle_deg=35.0)
    mvn, nclus, dpf, dx, dy = synth.synth_qm_state(dimx, dimy, seed=seed, k=8, p_out=0.5, p_wrong=0.4)
    zero = np.zeros((dimy, dimx), bool)
    zero[10:22, 15:33] = True
    zero[5, 5] = zero[40, 50] = zero[0, 0] = zero[dimy - 1, dimx - 1] = zero[30, 7] = True
    xy[zero.reshape(-1), 4:6] = 0.0
    empty = np.zeros((dimy, dimx), bool)
    empty[35, 20] = empty[36, 21] = empty[44, 44] = True
    nclus = nclus.copy()
    nclus[empty.reshape(-1)] = 0
    mvn = mvn.copy()
    mvn[empty.reshape(-1), :, :] = 0.0          # fraction 0 < 0.6: masked, with no candidate
    dpf = dpf.copy()
    dpf[empty] = 0
    ruv = disc_ruv(5.0)
    return (dpf, dx, dy, ruv, mvn, nclus, xy), zero, empty


def qm_tie_case():
    """Ties at the ABI: cluster lists with identical rows, and cluster pairs 0.01 px apart.

    Grid of constant ground (4, -4) with isolated masked points (further apart than the radius, so they do not see
    each other; the fit at each is the ground plus alpha times its own offset).  Per point the cluster list and the
    pick; the expected outcome follows from the strict `<` of the nearest-candidate loop (:2167-2180, the lower id wins
    a tie) and from the `< 0.0001` no-move rule (:2190) and is asserted by the CPU test on the oracle:
      dup_far     pick 2 far away, rows 0 and 1 identical and nearest        -> moves to id 0, never 1
      dup_current rows 0 and 1 identical, pick 1, both nearest               -> stays 1 (distance 0 < 0.0001)
      near_*      two clusters d apart along u, pick the farther one, for d = f32(0.01) and its neighbours and for
                  d with d*d just below / at / above 0.0001 in f64 -- moves iff (gu-qu)^2 >= 0.0001 in f64."""
    dimx, dimy = 48, 9
    ruv = disc_ruv(2.0)
    c = QmCase("ties", dimx, dimy, ruv, const_grid(dimx, dimy, 1500.0, 900.0), kmax=4)
    gx, gy = c.ground
    pts = {}
    u = 3
    c.set_point(u, 4, [(F32(gx + 0.125), F32(gy)), (F32(gx + 0.125), F32(gy)), (F32(gx + 3.0), F32(gy + 1.0))], 2); pts["dup_far"] = (u, 4)
    u += 4
    c.set_point(u, 4, [(F32(gx + 0.125), F32(gy)), (F32(gx + 0.125), F32(gy)), (F32(gx + 3.0), F32(gy + 1.0))], 1); pts["dup_current"] = (u, 4)
    base = F32(gx)
    d0 = F32(0.01)
    seps = [d0, np.nextafter(d0, F32(0)), np.nextafter(d0, F32(1)), F32(0.0078125), F32(0.015625)]
    # separations as differences of f32 numbers near 4: multiples of 2^-21; around 0.01 these straddle 0.0001 in f64
    kk = int(round(0.01 * 2 ** 21))
    seps += [F32(k * 2.0 ** -21) for k in range(kk - 3, kk + 4)]
    for i, d in enumerate(seps):
        u += 3
        near = base                                    # the ground itself: nearest to the fit
        far = F32(base + d)
        c.set_point(u, 4, [(near, F32(gy)), (far, F32(gy))], 1)
        pts[f"near_{i}"] = (u, 4)
    assert u + 2 < dimx
    return c, pts


# =====================================================================================================================
# clustering: the 0.5 px threshold where the f32 roundings decide
# =====================================================================================================================
def written_f32(ddx, ddy):
    """ddx*ddx + ddy*ddy as C evaluates it on floats without contraction: each product and the sum rounded to f32
    (the independent statement of MIMC_module.c:1154-1156)."""
    ddx = np.asarray(ddx, F32); ddy = np.asarray(ddy, F32)
    return (ddx * ddx).astype(F32) + (ddy * ddy).astype(F32)


def fused_f32(ddx, ddy):
    """fma(ddx, ddx, ddy*ddy): exact ddx^2 plus the rounded ddy^2, rounded once.  Exact in f64 for |dd| in [2^-5, 1)."""
    ddx = np.asarray(ddx, F32); ddy = np.asarray(ddy, F32)
    return (ddx.astype(np.float64) ** 2 + (ddy * ddy).astype(F32).astype(np.float64)).astype(F32)


def exact_f64(ddx, ddy):
    ddx = np.asarray(ddx, np.float64); ddy = np.asarray(ddy, np.float64)
    return ddx * ddx + ddy * ddy


THRESHOLD_CLASSES = ("written_lt_fused_ge", "written_ge_fused_lt", "written_eq", "written_vs_f64", "ulp_neighbours")


def threshold_pairs(per_class=64, seed=1154):
    """{class: (ddx [n], ddy [n]) f32}, both components non-zero, at least per_class pairs each."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ddx = rng.uniform(0.05, 0.4975, 600000).astype(F32)
    ddy = np.sqrt(np.maximum(0.25 - ddx.astype(np.float64) ** 2, 0)).astype(F32)
    ddy = (ddy.view(np.int32) + rng.integers(-3, 4, ddy.size).astype(np.int32)).view(F32)
    keep = (ddy > 0.03125) & (ddx > 0.03125)
    ddx, ddy = ddx[keep], ddy[keep]
    sgn = rng.integers(0, 4, ddx.size)
    ddx = np.where(sgn & 1, -ddx, ddx).astype(F32); ddy = np.where(sgn & 2, -ddy, ddy).astype(F32)
    q = F32(0.25)
    w, f, e = written_f32(ddx, ddy), fused_f32(ddx, ddy), exact_f64(ddx, ddy)
    sel = {
        "written_lt_fused_ge": (w < q) & (f >= q),
        "written_ge_fused_lt": (w >= q) & (f < q),
        "written_eq": w == q,
        "written_vs_f64": (w < q) != (e < 0.25),
    }
    out = {}
    for name, m in sel.items():
        idx = np.nonzero(m)[0][:per_class]
        out[name] = (ddx[idx].copy(), ddy[idx].copy())
    # +-1 ulp in ddy around the first per_class / 4 pairs of each class
    ux, uy = [], []
    for name in sel:
        x, y = out[name]
        for step in (-1, 1):
            ux.append(x[:per_class // 4 + 1]); uy.append((y[:per_class // 4 + 1].view(np.int32) + step).view(F32))
    out["ulp_neighbours"] = (np.concatenate(ux), np.concatenate(uy))
    return out


PAIR_SLOTS = ((0, 1), (31, 32), (0, 63), (62, 63))


def threshold_candidates(pairs, ndp=64):
    """dp [ndp][N][3] (ndp = 64: the slots are PAIR_SLOTS; smaller ndp: the last two slots move to ndp - 1, ndp - 2) with one pair per grid point, N = all pairs of all classes, and per point what the test needs:
    (dp, ddx, ddy, others) -- `others` = the number of further, far-away singleton clusters at the point.
    Pair i sits in the slots PAIR_SLOTS[i % 4]; the remaining slots are gated off (ncc 0.05 <= 0.1) for even i and
    far-away singletons (10 px apart) for odd i.  The first of the two is at (x0, y0) with x0 + ddx and y0 + ddy exact in
    f32, so that the kernel's subtraction returns ddx, ddy themselves (checked here)."""
    ddx = np.concatenate([pairs[c][0] for c in THRESHOLD_CLASSES])
    ddy = np.concatenate([pairs[c][1] for c in THRESHOLD_CLASSES])
    n = ddx.size
    dp = np.zeros((ndp, n, 3), F32)
    dp[:, :, 2] = 0.05
    others = np.zeros(n, np.int32)
    assert 34 <= ndp <= 64
    for i in range(n):
        a, b = [min(t, ndp - 64 + t) if t >= 62 else t for t in PAIR_SLOTS[i % 4]]
        x0, y0 = F32(0), F32(0)
        for cx, cy in ((F32(0.125), F32(-0.0625)), (F32(-0.25), F32(0.125))):
            if F32(F32(cx + ddx[i]) - cx) == ddx[i] and F32(F32(cy + ddy[i]) - cy) == ddy[i]:
                x0, y0 = cx, cy
                break
        x1, y1 = F32(x0 + ddx[i]), F32(y0 + ddy[i])
        assert F32(x1 - x0) == ddx[i] and F32(y1 - y0) == ddy[i] and F32(x0 - x1) == -ddx[i] and F32(y0 - y1) == -ddy[i]
        if i % 2:
            k = np.arange(ndp)
            dp[:, i, 0] = 100.0 + 10.0 * k
            dp[:, i, 1] = -50.0
            dp[:, i, 2] = 0.9
            others[i] = ndp - 2
        dp[a, i] = (x0, y0, 0.9)
        dp[b, i] = (x1, y1, 0.9)
    return dp, ddx, ddy, others


# =====================================================================================================================
# clustering: wave-shaped edges, odd values, statistics
# =====================================================================================================================
WAVE_NDP = (1, 2, 31, 32, 33, 63, 64)
WAVE_N = (1, 63, 64, 65, 129)


def wave_candidates(ndp, n, seed):
    """Clustered candidates: a few centres per point, 0.12 px noise, a third gated off."""
    rng = np.random.Generator(np.random.PCG64(1000 * ndp + n + seed))
    centre = rng.integers(0, 4, (ndp, n))
    dp = np.empty((ndp, n, 3), F32)
    dp[:, :, 0] = centre * 0.9 + rng.normal(0, 0.12, (ndp, n))
    dp[:, :, 1] = -centre * 0.3 + rng.normal(0, 0.12, (ndp, n))
    dp[:, :, 2] = np.where(rng.random((ndp, n)) < 0.33, 0.05, rng.uniform(0.2, 1.0, (ndp, n)))
    return dp


def shaped_components():
    """dp [64][N][3], one shape per grid point (names in order)."""
    names, cols = [], []

    def add(name, x, y=None, ncc=None):
        col = np.zeros((64, 3), F32)
        col[:, 0] = x
        col[:, 1] = 0.0 if y is None else y
        col[:, 2] = 0.9 if ncc is None else ncc
        names.append(name); cols.append(col)

    k = np.arange(64)
    add("singletons_64", 3.0 * k)
    rng = np.random.Generator(np.random.PCG64(63))
    rank = np.concatenate([[0], 1 + rng.permutation(63)])          # candidate 0 is one end: one new member per round
    add("chain_63_rounds", 0.4 * rank)
    add("chain_in_order", 0.4 * k)
    add("chain_reversed", 0.4 * k[::-1])
    add("two_interleaved_chains", np.where(k % 2 == 0, 0.4 * (k // 2), 100.0 + 0.4 * (k // 2)))
    add("two_interleaved_second_first", np.where(k % 2 == 1, 0.4 * (k // 2), 100.0 + 0.4 * (k // 2)))
    add("bridge_31_32", np.where(k < 31, 0.0, np.where(k == 31, 0.4, np.where(k == 32, 0.8, 1.2))))
    add("no_bridge_31_32", np.where(k < 32, 0.0, 1.2))
    add("all_one_place", np.full(64, 7.25))
    gate = np.full(64, 0.9, F32)
    gate[::2] = F32(0.1)                                            # exactly the gate: strict >, dropped
    gate[1::4] = np.nextafter(F32(0.1), F32(1))                     # its successor: kept
    add("ncc_at_gate", 0.7 * (k % 3), ncc=gate)
    add("only_lane_63", 0.0, ncc=np.where(k == 63, 0.9, 0.0))
    add("only_lane_32", 0.0, ncc=np.where(k == 32, 0.9, 0.0))
    add("none_valid", 0.0, ncc=np.full(64, 0.1, F32))
    big = np.where(k % 2 == 0, 1e20, -1e20)
    add("squares_overflow", big, y=np.where(k % 4 < 2, 3e19, -3e19))           # du^2 and dv^2 both overflow; 4 places
    add("near_f32_max", np.where(k % 2 == 0, 3e38, -3e38))          # the difference itself overflows
    return names, np.stack(cols, 1)


def nonfinite_components():
    """Points with NaN / +-Inf in du or dv and a passing ncc.  The reference is undefined here (a candidate that never
    labels itself indexes its sums at -1); DESIGN.md section 2 defines: it takes an id and carries nothing."""
    names, cols = [], []
    k = np.arange(64)

    def add(name, x, y):
        col = np.zeros((64, 3), F32)
        col[:, 0] = x; col[:, 1] = y; col[:, 2] = 0.9
        names.append(name); cols.append(col)

    base = (0.4 * (k % 5)).astype(F32)
    for name, val in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        for where in ("first", "last", "lane31_32", "every_third", "all"):
            x, y = base.copy(), np.zeros(64, F32)
            sel = {"first": k == 0, "last": k == 63, "lane31_32": (k == 31) | (k == 32), "every_third": k % 3 == 0,
                   "all": k >= 0}[where]
            x[sel] = val
            add(f"{name}_du_{where}", x, y)
            x, y = base.copy(), np.zeros(64, F32)
            y[sel] = val
            add(f"{name}_dv_{where}", x, y)
    x = base.copy(); x[3] = np.inf; x[9] = -np.inf; x[11] = np.nan
    add("mixed", x, np.zeros(64, F32))
    return names, np.stack(cols, 1)


def cancellation_candidates(seed=7):
    """Tight clusters far from zero: sxx / n - mean^2 in f32 loses every bit, or goes negative.  One grid point per
    (mean, sigma, count); counts 1..64, remaining slots gated off; every fourth point exact duplicates."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = []
    for mean in (100.0, 1000.0, 20000.0):
        for sigma in (0.01, 0.03, 0.06):
            for cnt in range(1, 65):
                col = np.zeros((64, 3), F32)
                col[:, 2] = 0.05
                slots = rng.permutation(64)[:cnt]
                if cnt % 4 == 0:
                    u, v = mean + rng.normal(0, sigma), -mean + rng.normal(0, sigma)
                else:
                    u, v = mean + rng.normal(0, sigma, cnt), -mean + rng.normal(0, sigma, cnt)
                col[slots, 0] = u; col[slots, 1] = v; col[slots, 2] = 0.9
                cols.append(col)
    return np.stack(cols, 1)


# =====================================================================================================================
# dpf0: fractions at the ratio
# =====================================================================================================================
def dpf0_fraction_case(ndp):
    """For every count c = 1..ndp: ratio = f32(c) / f32(ndp), and three points whose only cluster has the fraction
    ratio itself (strict >: not chosen), its f32 predecessor (not chosen) and its successor (chosen) -- plus points with
    two clusters above (the first wins), one below then one above (id 1), and an empty list.
    Returns [(ratio, mvn [N][3][5], nclus [N], expected dpf [N])]; expected is the plain numpy f32 statement."""
    out = []
    for c in range(1, ndp + 1):
        ratio = F32(c) / F32(ndp)
        lo, hi = np.nextafter(ratio, F32(0)), np.nextafter(ratio, F32(2))
        rows = [([ratio], 1), ([lo], 1), ([hi], 1), ([hi, hi], 2), ([lo, hi], 2), ([ratio, lo, hi], 3), ([hi], 0), ([], 0),
                ([lo, ratio], 2)]
        mvn = np.zeros((len(rows), 3, 5), F32)
        nclus = np.zeros(len(rows), np.int32)
        exp = -np.ones(len(rows), np.int32)
        for i, (fr, nc) in enumerate(rows):
            for j, f in enumerate(fr):
                mvn[i, j] = (1.0 + j, -1.0, 0.0, 0.0, f)
            nclus[i] = nc
            for j in range(nc):
                if F32(mvn[i, j, 4]) > ratio:
                    exp[i] = j
                    break
        out.append((float(ratio), mvn, nclus, exp))
    return out


# =====================================================================================================================
# dpf1
# =====================================================================================================================
def dpf1_inputs(dimx, dimy, seed, k=8, p_out=0.5, ang=35.0, radius=3.0):
    """(xy, ruv, dp) of the kind test_n1_parity uses; mvn / nclus / dpf0 come from the oracle in the tests."""
    from mimc3_amd import synth
    xy = synth.make_grid(dimx, dimy, 60, 60, 20, 20, 1806.0, angle_deg=ang)
    dp = synth.synth_candidates(dimx, dimy, seed=seed, k=k, p_out=p_out)
    dp[:, ::7, 2] = 0.05
    return xy, disc_ruv(radius), dp


def zero_apriori(xy, dimx, dimy, patch, singles):
    xy = xy.copy()
    z = np.zeros((dimy, dimx), bool)
    (v0, v1, u0, u1) = patch
    z[v0:v1, u0:u1] = True
    for v, u in singles:
        z[v, u] = True
    xy[z.reshape(-1), 4:6] = 0.0
    return xy, z


ISLAND = (slice(11, 15), slice(13, 19))          # of never_filled_island: 5 points of moat on every side, radius 3


def dpf1_cases(oracle):
    """[(name, dpf0, ruv, mvn, nclus, xy, reference_defined)].  mvn / nclus / dpf0 are the oracle's own clustering of
    synthetic candidates unless the case says otherwise.  The reference is defined on all of them: a zero a-priori is
    plain float arithmetic there (0/0 -> NaN direction weights, which never pass the threshold; v4/0 -> +Inf in the
    ratio column, which is then the maximum and excluded), and dimx or dimy below 3 only make its 3 x 3 smoothing loops
    empty.  The flag is kept for inputs that leave the reference's definition."""
    cases = []

    def base(dimx, dimy, seed, **kw):
        xy, ruv, dp = dpf1_inputs(dimx, dimy, seed, **kw)
        mvn, nclus = oracle.cluster_candidates(dp, kmax=dp.shape[0])
        d0 = oracle.get_dpf0(mvn, nclus, dimx, dimy, 0.6)
        return xy, ruv, mvn, nclus, d0

    # zero a-priori: a patch and single points, open (target) and assigned (neighbour) alike
    xy, ruv, mvn, nclus, d0 = base(40, 30, 31)
    xyz, _ = zero_apriori(xy, 40, 30, (8, 15, 10, 22), [(0, 0), (29, 39), (20, 5), (3, 33), (25, 25)])
    cases.append(("zero_apriori_patch", d0, ruv, mvn, nclus, xyz, True))
    xy, ruv, mvn, nclus, d0 = base(33, 21, 32, ang=-120.0, p_out=0.6)
    xyz, _ = zero_apriori(xy, 33, 21, (0, 0, 0, 0), [(v, u) for v in range(1, 21, 4) for u in range(2, 33, 5)])
    cases.append(("zero_apriori_singles", d0, ruv, mvn, nclus, xyz, True))
    # open points that can never be filled: an island of open points behind a moat of points without any cluster
    xy, ruv, mvn, nclus, d0 = base(36, 28, 33)
    nclus = nclus.copy(); d0 = d0.copy(); mvn = mvn.copy()
    moat = np.zeros((28, 36), bool); moat[6:20, 8:24] = True
    isle = np.zeros((28, 36), bool); isle[ISLAND] = True
    ring = moat & ~isle
    nclus[ring.reshape(-1)] = 0; mvn[ring.reshape(-1)] = 0; d0[ring] = -1
    d0[isle] = -1
    nclus[isle.reshape(-1)] = np.maximum(nclus[isle.reshape(-1)], 1)
    cases.append(("never_filled_island", d0, ruv, mvn, nclus, xy, True))
    # a neighbour list so short that the first level is already below 3: nothing is interpolated
    xy, ruv, mvn, nclus, d0 = base(20, 15, 34)
    cases.append(("nn_3", d0, np.array([(0, 0), (1, 0), (0, 1)], np.int32), mvn, nclus, xy, True))
    cases.append(("nn_4", d0, np.array([(-1, 0), (0, 0), (1, 0), (0, 1)], np.int32), mvn, nclus, xy, True))
    # no interior for the 3 x 3 smoothing
    for dimx, dimy in ((1, 40), (40, 1), (2, 33), (33, 2), (3, 29), (29, 3), (1, 1), (2, 2), (3, 3)):
        xy, ruv, mvn, nclus, d0 = base(dimx, dimy, 35 + dimx + 2 * dimy, p_out=0.55)
        cases.append((f"thin_{dimx}x{dimy}", d0, ruv, mvn, nclus, xy, True))
    # duplicate cluster rows at open points: the snap takes the lower id
    xy, ruv, mvn, nclus, d0 = base(30, 24, 36)
    mvn = mvn.copy(); nclus = nclus.copy()
    op = np.nonzero((d0.reshape(-1) < 0) & (nclus > 0) & (nclus < mvn.shape[1]))[0]
    for g in op:
        n = nclus[g]
        mvn[g, 1:n + 1] = mvn[g, 0:n].copy()        # row 0 twice, the others shifted up
        nclus[g] = n + 1
    cases.append(("duplicate_rows", d0, ruv, mvn, nclus, xy, True))
    return cases


# =====================================================================================================================
# the whole chain: clustering -> dpf0 -> dpf1 -> QM on one tensor that mixes the edges above
# =====================================================================================================================
def chain_case(dimx=60, dimy=45, ndp=40):
    """(dp [ndp][N][3], xy, dimx, dimy, meter_per_spacing): noise candidates with, scattered over the grid, the
    threshold pairs of every class, points whose largest cluster holds exactly 24 / 40 = 0.6f of the candidates (not
    chosen by dpf0), 25 / 40 (chosen) and 23 / 40, and a patch plus single points of zero a-priori velocity."""
    from mimc3_amd import synth
    xy = synth.make_grid(dimx, dimy, 60, 60, 20, 20, 1806.0, angle_deg=37.0)
    mps = float(F32(xy[1, 0] - xy[0, 0]))
    dp = synth.synth_candidates(dimx, dimy, seed=44, k=ndp, p_out=0.5)
    n = dimx * dimy
    tp, _, _, _ = threshold_candidates(threshold_pairs(), ndp)
    rng = np.random.Generator(np.random.PCG64(45))
    where = rng.permutation(n)
    at = where[:tp.shape[1]]
    dp[:, at] = tp
    k = np.arange(ndp)
    for j, g in enumerate(where[tp.shape[1]:tp.shape[1] + 90]):
        cnt = (24, 25, 23)[j % 3]
        dp[:, g, 0] = np.where(k < cnt, 4.0 + 0.01 * (k % 3), 30.0 + 5.0 * k)
        dp[:, g, 1] = np.where(k < cnt, -4.0, 12.0)
        dp[:, g, 2] = 0.9
    xy, _ = zero_apriori(xy, dimx, dimy, (12, 20, 30, 44), [(2, 3), (40, 50), (44, 0), (22, 22)])
    return dp, xy, dimx, dimy, mps


def oracle_chain(oracle, dp, xy, dimx, dimy, mps, dt=16.0, mpp=15.0):
    """mimc2_postprocess from the oracle's stages, as test_vmap_parity.test_postprocess_vs_oracle chains them.
    Returns (planes [5][N], dpf0, QM stats)."""
    ndp = dp.shape[0]
    mvn, nclus = oracle.cluster_candidates(dp, kmax=ndp)
    d0 = oracle.get_dpf0(mvn, nclus, dimx, dimy, 0.6)
    d1, x1, y1 = oracle.get_dpf1(d0, oracle.get_ruv_neighbor(xy, dimx, dimy, mps, 3.0), mvn, nclus, xy, dt, mpp)
    d2, _, _, st = oracle.qm(d1, x1, y1, oracle.get_ruv_neighbor(xy, dimx, dimy, mps, 5.0), mvn, nclus, xy)
    d2 = d2.reshape(-1)
    n = dimx * dimy
    want = np.full((5, n), np.nan, F32)
    ok = d2 >= 0
    want[:, ok] = mvn[np.arange(n)[ok], d2[ok], :].T
    return want, d0, st
