"""The u8 matcher step behind u8_classify (u8_classify_kernel.hip): one classification pass per call, the matrix-core kernel over
the clean list, the register-tiled kernel over the rest list (with the points the matrix-core launch appended).  GPU: path "auto"
against the register-tiled kernel alone ("u8px") bit for bit, and against the port oracle on the small cases, at every chip size of
the program and in both directions, on the inputs that aim at the lists: one of them empty, list lengths around a wave and not a
multiple of 8 (the XCD order of list positions), static and dynamic hand-ons, long climbs on a stripe image, the two matcher lanes, a pair
change and a path change between calls.  CPU: the point classes of BASELINE C2 from a numpy summed-area table."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from mimc3_amd import synth
from u8_stats_common import stats_run

OCWS = (7, 15, 16, 30, 40)
C2_CLASSES = (96939, 67608, 20928, 14525)          # clean, window nulls only, chip nulls only, both


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check(ctx, oracle, i0, i1, xy, offset, off, uv, ocw, what, with_oracle=True):
    """auto == u8px (== the oracle) in both directions; auto took the matrix-core path"""
    offset = np.asarray(offset, np.int32)
    for swap in (False, True):
        o, p = (-offset, -uv) if swap else (offset, uv)
        ctx.set_path("auto")
        got = ctx.matching_ncc_dlc_2(xy, o, off, p, ocw, swap=swap)
        assert ctx.last_path() == "u8_mfma", what
        ctx.set_path("u8px")
        assert_bits_equal(got, ctx.matching_ncc_dlc_2(xy, o, off, p, ocw, swap=swap), f"{what} swap {swap}: auto vs u8px")
        if with_oracle:
            a, b = (i1, i0) if swap else (i0, i1)
            assert_bits_equal(got, oracle.match(a, b, xy, o, off, p, ocw), f"{what} swap {swap}: auto vs oracle")
    ctx.set_path("auto")


def small(ocw, seed, **kw):
    kw.setdefault("h", 2 * ocw + 230)
    kw.setdefault("w", 2 * ocw + 240)
    kw.setdefault("dimx", 6)
    kw.setdefault("dimy", 5)
    return synth.make_small(seed=seed, ocw=ocw, shift=kw.pop("shift", (3, -2)), angle_deg=kw.pop("angle_deg", 40.0),
                            speed=kw.pop("speed", 1700.0), noise_dn=2, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_null_free_pair_rest_list_empty(api, oracle, ocw):
    c = small(ocw, 8100 + ocw, null_frac=0.0, offset=(1, -2))
    assert (c.i0 != 0).all() and (c.i1 != 0).all()
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        check(ctx, oracle, c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw, f"null-free ocw {ocw}")


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_every_window_holds_a_null_clean_list_empty(api, oracle, ocw):
    """a null every 8 pixels in both images: no window (>= 18 pixels wide) and no chip is null-free"""
    c = small(ocw, 8200 + ocw, null_frac=0.0)
    c.i0[::8, ::8] = 0.0
    c.i1[::8, ::8] = 0.0
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        check(ctx, oracle, c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw, f"all-null ocw {ocw}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 77])
@pytest.mark.parametrize("ocw", OCWS)
def test_list_lengths_around_a_wave_and_not_a_multiple_of_8(api, oracle, ocw, n):
    c = small(ocw, 8300 + ocw, null_frac=0.04, dimx=11, dimy=7, h=2 * ocw + 260, w=2 * ocw + 300)
    xy = np.ascontiguousarray(c.xyuvav[:n])
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(xy, c.dt, c.mpp, ocw, H, W)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        check(ctx, oracle, c.i0, c.i1, xy, c.offset, off, uv, ocw, f"N {n} ocw {ocw}")


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_static_and_dynamic_hand_ons(api, oracle, ocw):
    """every ninth point 3.4 times as fast (corridors wider than the tile: the classifier's kMxRest) among slow ones; and a field of
    17 to 29 pivots whose shift lies far off the corridor (tiles that do not cover the cell grid: climbs leave them)"""
    c = small(ocw, 8400 + ocw, null_frac=0.02, shift=(3, -4), angle_deg=-50.0, speed=1600.0, h=2 * ocw + 400, w=2 * ocw + 410,
              dimx=7, dimy=7, margin=ocw + 120)
    xy = c.xyuvav.copy()
    xy[::9, 4:6] *= 3.4
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(xy, c.dt, c.mpp, ocw, H, W)
    last = np.abs(uv[off[1:] - 1]).max(axis=1)
    assert last.max() > 29 and np.median(last) <= 20, (last.max(), np.median(last))
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        check(ctx, oracle, c.i0, c.i1, xy, c.offset, off, uv, ocw, f"mixed field ocw {ocw}")
    i0, i1, xy, offset, off, uv = off_corridor_case(api, ocw)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check(ctx, oracle, i0, i1, xy, offset, off, uv, ocw, f"off-corridor shift ocw {ocw}")


def stripes(H, W, seed):
    """images of x alone (as tests/test_ncc_ties.py): every scan ties in v, the climbs run on past the 16 recorded scans"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = np.convolve(rng.standard_normal(W + 40), np.ones(5) / 5, mode="same")[20:W + 20]
    f = np.clip(np.rint(128 + 40 * f / f.std()), 1, 255)
    g = np.clip(np.roll(f, 2) + rng.integers(-3, 4, size=W), 1, 255)
    return np.tile(f, (H, 1)).astype(np.float32), np.tile(g, (H, 1)).astype(np.float32)


def stripe_case(ocw):
    """1,190 null-free points on a stripe image, with pivot sets that make long climbs"""
    reach, nx, ny = 15, 35, 34
    sp, m = 2 * (ocw + reach) + 3, ocw + reach + 4
    g = np.arange(nx * ny)
    xy = np.zeros((nx * ny, 6))
    xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3] = g % nx, g // nx, m + (g % nx) * sp, m + (g // nx) * sp
    H, W = 2 * m + (ny - 1) * sp + 1, 2 * m + (nx - 1) * sp + 1
    i0, i1 = stripes(H, W, 8500 + ocw)
    lists = [[(1, 0), (0, 12)], [(k, 0) for k in range(8)], [(k, k // 2) for k in range(-4, 12)]]
    piv = [lists[k % 3] for k in range(nx * ny)]
    off = np.zeros(nx * ny + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in piv])
    uv = np.ascontiguousarray(np.concatenate([np.array(p, np.int32).reshape(-1, 2) for p in piv]), np.int32)
    return i0, i1, xy, np.array([1, -1], np.int32), off, uv


def off_corridor_case(api, ocw):
    """17 to 29 pivots and a shift far off the corridor: tiles that do not cover the cell grid, climbs that leave them"""
    c = small(ocw, 8450 + ocw, null_frac=0.03, shift=(9, 7), angle_deg=45.0, speed=2900.0, h=2 * ocw + 300, w=2 * ocw + 310,
              dimx=6, dimy=6, margin=ocw + 80)
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    assert 15 <= int(np.abs(uv[off[1:] - 1]).max()) <= 29
    return c.i0, c.i1, c.xyuvav, c.offset, off, uv


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_long_climbs_on_a_stripe_image(api, oracle, ocw):
    """the stripe case: every point is on the clean list (1,190 list positions: the XCD order over more than a thousand workgroups);
    whatever the matrix-core launch hands on itself is appended to the rest list (test_hand_on_accounting counts it: none at ocw 7);
    the oracle on the first rows of the grid"""
    i0, i1, xy, offset, off, uv = stripe_case(ocw)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check(ctx, oracle, i0, i1, xy, offset, off, uv, ocw, f"stripes ocw {ocw}", with_oracle=False)
        ctx.set_path("auto")
        got = ctx.matching_ncc_dlc_2(xy, offset, off, uv, ocw)
    n = 70
    assert_bits_equal(got[:n], oracle.match(i0, i1, np.ascontiguousarray(xy[:n]), offset, off[:n + 1], uv[:off[n]], ocw), "stripes vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
@pytest.mark.parametrize("case", ["stripes", "off_corridor"])
def test_hand_on_accounting(case, ocw):
    """what the matrix-core launch does not finish of its clean list is exactly what is classed kMxRest beyond the classifier's rest
    list afterwards: no point lost, none taken twice.  The count is printed; that the append path is really taken is asserted on
    BASELINE C2 (test_c2_classifier_counts_equal_numpy), where dozens of climbs leave the tile -- on the stripe image at ocw 7 none
    does (measured: 1,190 listed, 1,190 finished), so these two cases prove the accounting, not the append"""
    body = ("ocw = %d; i0, i1, xy, offset, off, uv = t.stripe_case(ocw)" if case == "stripes" else
            "ocw = %d; i0, i1, xy, offset, off, uv = t.off_corridor_case(api, ocw)") % ocw
    c_clean, c_rest, c_nulls, c_wn, l_clean, l_rest, done, rest_after = stats_run(body)
    print(case, ocw, "clean list", l_clean, "finished", done, "rest list", l_rest, "kMxRest after the launch", rest_after)
    assert (c_clean, c_rest, c_nulls + c_wn) == (l_clean, l_rest, 0)
    assert 0 <= l_clean - done == rest_after - l_rest


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_two_matcher_lanes_back_to_back(api, ocw):
    """42,000 points through matching_ncc_dlc_cor: three chunks on two streams and two matcher lanes (their lists must not alias),
    twice back to back, against the register-tiled kernel alone and against the resident-list entry"""
    c = synth.make_small(seed=8600 + ocw, ocw=ocw, shift=(3, -2), angle_deg=25.0, speed=1500.0, h=1230, w=1280, dimx=210, dimy=200,
                         noise_dn=2, null_frac=0.02, margin=ocw + 40)
    assert c.xyuvav.shape[0] >= 40000
    H, W = c.i0.shape
    cor = api.pivot_corridors(c.xyuvav, c.dt, c.mpp)
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        ctx.set_path("u8px")
        want = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, ocw)
        want_sw = ctx.matching_ncc_dlc_2(c.xyuvav, -c.offset, off, -uv, ocw, swap=True)
        ctx.set_path("auto")
        for rep in range(2):
            assert_bits_equal(ctx.matching_ncc_dlc_cor(c.xyuvav, cor, c.offset, ocw), want, f"chunked call {rep}")
            assert ctx.last_path() == "u8_mfma"
            assert_bits_equal(ctx.matching_ncc_dlc_cor(c.xyuvav, cor, -c.offset, ocw, swap=True), want_sw, f"chunked call {rep}, swapped")
        assert_bits_equal(ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, ocw), want, "resident lists")


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", OCWS)
def test_pair_change_and_path_change_between_calls(api, oracle, ocw):
    a = small(ocw, 8700 + ocw, null_frac=0.05)
    b = small(ocw, 8750 + ocw, null_frac=0.0, shift=(-2, 4))
    H, W = a.i0.shape
    off, uv = api.get_uv_pivot(a.xyuvav, a.dt, a.mpp, ocw, H, W)
    with api.Context(0) as ctx:
        for c in (a, b, a):
            ctx.set_images(c.i0, c.i1)
            check(ctx, oracle, c.i0, c.i1, a.xyuvav, a.offset, off, uv, ocw, f"pair {c.name} ocw {ocw}")


def c2_classes(api, c, ocw):
    """(clean, window nulls only, chip nulls only, both) of the forward pass, from summed-area tables of the null masks"""
    H, W = c.i0.shape
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    last = uv[off[1:] - 1].astype(np.int64)
    pad = 256

    def table(img):
        z = np.zeros((H + 2 * pad + 1, W + 2 * pad + 1), np.int64)
        z[pad + 1:pad + H + 1, pad + 1:pad + W + 1] = (img == 0)
        return z.cumsum(0).cumsum(1)

    def box(S, x, y, w, h):
        x, y = x + pad, y + pad
        return S[y + h, x + w] - S[y, x + w] - S[y + h, x] + S[y, x]

    S0, S1 = table(c.i0), table(c.i1)
    u0, v0 = c.xyuvav[:, 2].astype(np.int64), c.xyuvav[:, 3].astype(np.int64)
    dx2, dy2 = np.abs(last[:, 0]) + ocw + 2, np.abs(last[:, 1]) + ocw + 2
    chip = box(S0, u0 - ocw, v0 - ocw, 2 * ocw + 1, 2 * ocw + 1)
    # the window's written area (MIMC_module.c:869-886): 2 dx2 x 2 dy2 pixels; null = the image's zeros (outside the image: its zero border)
    win = box(S1, u0 + c.offset[0] - dx2, v0 + c.offset[1] - dy2, 2 * dx2, 2 * dy2)
    inside = (u0 + c.offset[0] - dx2 >= 0) & (v0 + c.offset[1] - dy2 >= 0) & (u0 + c.offset[0] + dx2 <= W) & (v0 + c.offset[1] + dy2 <= H)
    assert inside.all()                                      # (C2: no window leaves the image, so the image's zeros are all the nulls)
    assert np.abs(last).max() <= 29 and np.diff(off).max() <= 64          # every pivot set fits the tile
    return (int(((win == 0) & (chip == 0)).sum()), int(((win != 0) & (chip == 0)).sum()), int(((win == 0) & (chip != 0)).sum()),
            int(((win != 0) & (chip != 0)).sum()))


def test_c2_point_classes_from_a_numpy_table(api):
    """CPU: the four class counts of BASELINE C2's forward pass on record"""
    c = synth.make_case("C2")
    assert c2_classes(api, c, 16) == C2_CLASSES


@pytest.mark.gpu
def test_c2_classifier_counts_equal_numpy(api):
    """GPU: the class bytes and list lengths as u8_classify leaves them on BASELINE C2 are numpy's four counts exactly (the null
    forms are off: the three null classes are all kMxRest); and every point is taken once -- what the matrix-core launch does not
    finish of its list (57 on record: a few dozen) is kMxRest afterwards"""
    want = c2_classes(api, synth.make_case("C2"), 16)
    body = 'c = synth.make_case("C2"); ocw = 16; i0, i1, xy, offset = c.i0, c.i1, c.xyuvav, c.offset; off, uv = api.get_uv_pivot(xy, c.dt, c.mpp, ocw, *i0.shape)'
    c_clean, c_rest, c_nulls, c_wn, l_clean, l_rest, done, rest_after = stats_run(body)
    print("u8_classify", (c_clean, c_rest), "finished", done, "kMxRest after the launch", rest_after, "numpy", want)
    assert (c_clean, c_rest, c_nulls, c_wn) == (want[0], sum(want[1:]), 0, 0)
    assert (l_clean, l_rest) == (want[0], sum(want[1:]))
    assert done + rest_after == sum(want)
    assert 0 < l_clean - done <= 200                              # dynamic hand-ons: dozens, not hundreds (0.2 % of the clean class at most)
