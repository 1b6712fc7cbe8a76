"""GPU: the coarse-to-fine exhaustive search on every pair class (mimc3_match_ncc_pyramid_dn: u8, u16 or f32 levels, one exhaustive
search per level, the chaining on the device, candidates at level 0) against its test-side definition (tests/pyramid_dn_oracle.py):
the levels exactly, the record as assert_records_match compares it (bit for bit but the SNR, within 1 f32 ulp), shift_out exactly,
the candidates bit for bit."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_dn_common import to_dn16
from full_search_common import assert_records_match
from mimc3_amd import synth
from pyramid_dn_oracle import as_class, case, dn12_low, pyramid_dn, pyramid_search_dn
from pyramid_oracle import BIG, big_case

pytestmark = pytest.mark.gpu

MX_OCW = (7, 15, 16, 30, 32, 40)
PATH = {"u8": "u8_mfma_full", "u16": "u16_full", "f32": "f32i_full"}
R = 6


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_levels(ctx, f0, f1, what, levels=(1, 2, 3)):
    """get_pyramid_level against the oracle's levels of the float images f0, f1, exactly."""
    p0, p1 = pyramid_dn(f0, max(levels) + 1), pyramid_dn(f1, max(levels) + 1)
    for lv in levels:
        l0, l1 = ctx.get_pyramid_level(lv)
        assert l0.shape == p0[lv].shape and l1.shape == p1[lv].shape
        assert_bits_equal(l0, p0[lv], f"{what}: image 0, level {lv}")
        assert_bits_equal(l1, p1[lv], f"{what}: image 1, level {lv}")


def check_border(ctx, H, W, xyuvav, path, what):
    """The level planes' borders are zero: every point's level-1 box starts on the first border column right of the level image (so the
    columns a row's last vector wrote are in it) and the level-0 box lies in the border too -- no arg-max on level 1 (d_0 = 2 d_1), -3."""
    ocw, h = 7, 7 + 1
    xy = np.ascontiguousarray(xyuvav, np.float64)
    u0 = xy[:, 2].astype(np.int64)
    d1 = (W >> 1) + h - (u0 >> 1)
    shift = np.stack([2 * d1, np.zeros_like(d1)], axis=1).astype(np.int32)
    rec, _, sh = ctx.match_ncc_pyramid_dn(xy, (0, 0), ocw, 1, 2, shift=shift)
    assert ctx.last_path() == path
    np.testing.assert_array_equal(sh, shift, what + ": level 1 found an arg-max in the border")
    assert (rec[:, 2] == -3).all(), what + f": statuses {rec[:, 2].tolist()}"


def class_of(f0, f1):
    """The class the library gives a pair: 8-bit, else scaled integers below 4096 (x 1 or x 8 per image), else integral f32."""
    if all((f == np.rint(f)).all() and f.max() <= 255 for f in (f0, f1)):
        return "u8"
    q = [f if (f == np.rint(f)).all() else f * np.float32(8) for f in (f0, f1)]
    return "u16" if all(v.max() < 4096 for v in q) else "f32"


def hand_pair(cls):
    """37 x 45 (odd; Wd = 22 is no multiple of a vector width): the value limit of the class, blocks with 0..4 nulls, sums that tie under
    (sum + n/2) / n for n = 2, 3, 4.  Image 0 holds integers (shift 0), image 1 multiples of 1/8 (shift 3; not on the 8-bit class)."""
    top = {"u8": 255, "u16": 4095, "f32": 2 ** 20 - 1}[cls]
    rng = np.random.default_rng(37)
    w = [rng.integers(1, top + 1, (37, 45)) for _ in range(2)]
    for a in w:
        a[rng.random((37, 45)) < 0.35] = 0                      # blocks with every null count
        a[0:2, 0:2] = top                                       # the limit: the mean of four is the limit
        a[0:2, 2:4] = [[top, 0], [0, top - 1]]                  # n = 2, an odd sum: ties up
        a[0:2, 4:6] = [[5, 6], [0, 9]]                          # n = 3: 20 + 1 -> 7
        a[0:2, 6:8] = [[5, 6], [0, 8]]                          # n = 3: 19 + 1 -> 6
        a[0:2, 8:10] = [[1, 2], [2, 1]]                         # n = 4: 6 + 2 -> 2
        a[0:2, 10:12] = [[0, 0], [0, 0]]
        a[0:2, 12:14] = [[0, 0], [3, 0]]
        a[2:4, 42:44] = [[top, top], [top, 0]]                  # the last whole block of a row
        a[34:36, 0:2] = [[top, 1], [0, 0]]                      # the last whole block of a column
        if cls == "f32":
            a[4:6, 0:2] = 65535
    i0 = w[0].astype(np.float32)
    i1 = w[1].astype(np.float32) if cls == "u8" else (w[1] / 8.0).astype(np.float32)
    nn = [((a[:36, :44].reshape(18, 2, 22, 2) != 0).sum(axis=(1, 3))) for a in w]
    assert all(set(np.unique(n).tolist()) == {0, 1, 2, 3, 4} for n in nn)
    return np.ascontiguousarray(i0), np.ascontiguousarray(i1)


# ---- 1. the reduction alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["u16", "f32"])
def test_levels_of_the_fixtures_and_their_filtered_forms(api, cls):
    c = case(16, 0.03, 8101)
    i0, i1 = as_class(cls, c)
    H, W = i0.shape
    seen = set()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check_levels(ctx, i0, i1, cls)
        check_border(ctx, H, W, c.xyuvav, PATH[cls], cls)
        for k in (2, 0):                                          # the Laplacian (shift 3) and gx (shift 0)
            ctx.filter_images(None)
            ctx.filter_images(api.CLI_KERNELS[k])
            f0, f1 = ctx.get_images(H, W)
            seen.add("shift0" if (f0 == np.rint(f0)).all() and (f1 == np.rint(f1)).all() else "shift3")
            check_levels(ctx, f0, f1, f"{cls}, kernel {k}")
            check_border(ctx, H, W, c.xyuvav, PATH[cls], f"{cls}, kernel {k}")
        ctx.filter_images(None)
        check_levels(ctx, i0, i1, cls + " again")
    assert seen == {"shift0", "shift3"}


def test_levels_of_an_8bit_pair(api):
    c = case(16, 0.03, 8101)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        check_levels(ctx, c.i0, c.i1, "u8")
        check_border(ctx, *c.i0.shape, c.xyuvav, PATH["u8"], "u8")


@pytest.mark.parametrize("cls", ["u8", "u16", "f32"])
def test_levels_at_the_value_limits(api, cls):
    i0, i1 = hand_pair(cls)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        check_levels(ctx, i0, i1, "hand-made " + cls)
        xy = np.zeros((1, 6))
        xy[0, 2:4] = (20, 18)
        check_border(ctx, 37, 45, xy, PATH[cls], "hand-made " + cls)
        with pytest.raises(api.Mimc3Error) as e:                # 37 >> 4 = 2, but level 5 does not exist; level 0 is not a level
            ctx.get_pyramid_level(5)
        assert e.value.code == -1
    tiny = np.full((7, 9), {"u8": 9, "u16": 300, "f32": 70000}[cls], np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(tiny, tiny)
        assert ctx.get_pyramid_level(2)[0].shape == (1, 2)
        with pytest.raises(api.Mimc3Error) as e:                # 7 >> 3 = 0: an empty level
            ctx.get_pyramid_level(3)
        assert e.value.code == -1


# ---- 2. oracle parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["u16", "f32"])
@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("null_frac", [0.0, 0.03, 0.15])
@pytest.mark.parametrize("ocw", MX_OCW)
def test_oracle_parity(api, ocw, null_frac, levels, cls):
    """Every chip size, null fraction and level count, both directions; match_ncc_full_dn at shift_out reproduces record and candidates."""
    c = case(ocw, null_frac, 8200 + ocw + int(100 * null_frac) + levels, levels)
    i0, i1 = as_class(cls, c, ocw)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    npk = (0, 4) if ocw in (7, 16, 40) else (0,)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for swap in (False, True):
            off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
            for npeaks in npk:
                what = f"{cls} ocw {ocw} nulls {null_frac} L {levels} swap {swap} npeaks {npeaks}"
                rec, cand, sh = ctx.match_ncc_pyramid_dn(c.xyuvav, off, ocw, R, levels, npeaks, shift=sh_in, swap=swap)
                assert ctx.last_path() == PATH[cls]
                want, want_cand, want_sh = pyramid_search_dn(i0, i1, c.xyuvav, off, ocw, R, levels, npeaks, shift=sh_in, swap=swap)
                np.testing.assert_array_equal(sh, want_sh, what)
                assert_records_match(rec, want, what)
                full = ctx.match_ncc_full_dn(c.xyuvav, off, ocw, R, npeaks, shift=sh, swap=swap)
                assert_bits_equal(full[0], rec, what + " vs match_ncc_full_dn")
                if npeaks:
                    assert_bits_equal(cand, want_cand, what + ": candidates")
                    assert_bits_equal(full[1], cand, what + ": candidates vs match_ncc_full_dn")
                else:
                    assert cand is None


# ---- 3. filtered pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["u8", "f32"])
def test_filtered_pairs(api, cls):
    """The three CLI kernels on an 8-bit pair (its Laplacian is a scaled-integer pair; a smooth pair's gradients may fit 8 bits again) and
    on a 16-bit pair: the levels are reductions of the filtered planes, and the oracle reads ctx.get_images() as they are."""
    c = case(16, 0.03, 8701, 2)
    i0, i1 = (c.i0, c.i1) if cls == "u8" else as_class("f32", c)
    H, W = i0.shape
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    seen, paths = set(), set()
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for k, kern in enumerate(api.CLI_KERNELS):
            ctx.filter_images(None)                               # fresh planes: what a filter leaves in the border is the next one's input
            ctx.filter_images(kern)
            f0, f1 = ctx.get_images(H, W)
            seen.add("shift0" if (f0 == np.rint(f0)).all() and (f1 == np.rint(f1)).all() else "shift3")
            for swap in (False, True):
                off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
                what = f"{cls} kernel {k} swap {swap}"
                rec, cand, sh = ctx.match_ncc_pyramid_dn(c.xyuvav, off, 16, R, 2, 4, shift=sh_in, swap=swap)
                assert ctx.last_path() == PATH[class_of(f0, f1)]
                paths.add(ctx.last_path())
                want, want_cand, want_sh = pyramid_search_dn(f0, f1, c.xyuvav, off, 16, R, 2, 4, shift=sh_in, swap=swap)
                np.testing.assert_array_equal(sh, want_sh, what)
                assert_records_match(rec, want, what)
                assert_bits_equal(cand, want_cand, what + ": candidates")
        ctx.filter_images(None)
    assert seen == {"shift0", "shift3"}
    assert PATH["u16" if cls == "u8" else "f32"] in paths


# ---- 4. an 8-bit pair through the new entry -------------------------------------------------------------------------------------------
def test_8bit_pair_is_match_ncc_pyramid(api):
    c = case(16, 0.03, 8101)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for levels in (1, 2, 3):
            for swap in (False, True):
                off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
                want, want_sh = ctx.match_ncc_pyramid(c.xyuvav, off, 16, 9, levels, shift=sh_in, swap=swap)
                rec, none, sh = ctx.match_ncc_pyramid_dn(c.xyuvav, off, 16, 9, levels, shift=sh_in, swap=swap)
                assert none is None and ctx.last_path() == PATH["u8"]
                np.testing.assert_array_equal(sh, want_sh)
                assert_bits_equal(rec, want, f"L {levels} swap {swap}")
                out, cand, sh4 = ctx.match_ncc_pyramid_dn(c.xyuvav, off, 16, 9, levels, 4, shift=sh_in, swap=swap)
                np.testing.assert_array_equal(sh4, want_sh)
                assert_bits_equal(out, want, f"L {levels} swap {swap}, npeaks 4: record")
                o2, c2 = ctx.match_ncc_full_multi(c.xyuvav, off, 16, 9, 4, shift=sh4, swap=swap)
                assert_bits_equal(out, o2, "record vs match_ncc_full_multi")
                assert_bits_equal(cand, c2, "candidates vs match_ncc_full_multi")


# ---- 5. large displacement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["u16", "f32"])
def test_large_displacement(api, cls):
    """(+70, -45) px with no prior: one level at R 15 finds it at under 10 % of the points, three levels at >= 90 % of the valid ones."""
    b0, b1, g = big_case()
    i0, i1 = (dn12_low(b0, 51), dn12_low(b1, 52)) if cls == "u16" else (to_dn16(b0, 51), to_dn16(b1, 52))
    du, dv = BIG["motion"]
    ocw = BIG["ocw"]
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        one, _, sh1 = ctx.match_ncc_pyramid_dn(g, (0, 0), ocw, 15, 1)
        rec, _, sh = ctx.match_ncc_pyramid_dn(g, (0, 0), ocw, 15, 3)
        assert ctx.last_path() == PATH[cls]
    assert not sh1.any()
    hit1 = (np.abs(one[:, 0] - du) < 0.05) & (np.abs(one[:, 1] - dv) < 0.05)
    assert hit1.mean() < 0.1
    ok = rec[:, 2] >= -1
    hit = ok & (np.abs(rec[:, 0] - du) < 0.05) & (np.abs(rec[:, 1] - dv) < 0.05)
    assert ok.sum() > 0 and hit.sum() >= 0.9 * ok.sum()
    want, _, want_sh = pyramid_search_dn(i0, i1, g, (0, 0), ocw, 15, 3)
    np.testing.assert_array_equal(sh, want_sh)
    assert_records_match(rec, want, "(+70, -45)")
    assert_records_match(one, pyramid_search_dn(i0, i1, g, (0, 0), ocw, 15, 1)[0], "(+70, -45), one level")


# ---- 6. the remaining cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["u16", "f32"])
def test_boxes_beyond_the_zero_border(api, cls):
    """Points whose derived level-0 search box leaves the 256-px zero border get the all-NaN record and candidates; no refusal."""
    c = case(15, 0.0, 8301)
    i0, i1 = as_class(cls, c)
    shift = np.zeros((c.n, 2), np.int32)
    shift[::3] = (400, 0)                              # coarser levels search zeros (-3: no arg-max); level 0's boxes leave the border
    shift[1::3] = (0, -280)                            # level 0's boxes leave the border on the top row of points only
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        rec, cand, sh = ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), 15, 15, 3, 2, shift=shift)
        ok = ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), 15, 15, 3)[0]        # the context still works
    want, want_cand, want_sh = pyramid_search_dn(i0, i1, c.xyuvav, (0, 0), 15, 15, 3, 2, shift=shift)
    np.testing.assert_array_equal(sh, want_sh)
    assert_records_match(rec, want, "beyond the border")
    assert_bits_equal(cand, want_cand, "beyond the border: candidates")
    assert np.isnan(rec[::3]).all() and np.isnan(cand[:, ::3]).all()
    assert np.isnan(rec).all(axis=1).sum() > len(rec[::3])
    assert (ok[:, 2] >= -1).any()


def test_pair_changes(api):
    """16-bit, then 12-bit, then 8-bit, then filtered and unfiltered on one context: the levels are rebuilt each time, and every result
    is a fresh context's."""
    a, b = case(16, 0.03, 8401), case(16, 0.03, 8402)
    shift = api.prior_shift(b.xyuvav, b.dt, b.mpp)
    lap = api.CLI_KERNELS[2]
    pairs = [("f32", as_class("f32", a), None), ("f32", as_class("f32", b), None), ("u16", as_class("u16", b), None),
             ("u8", (b.i0, b.i1), None), ("u16", (b.i0, b.i1), lap), ("u8", (b.i0, b.i1), None), ("f32", as_class("f32", b), lap),
             ("f32", as_class("f32", b), None)]

    def run(ctx, cls, kern):
        ctx.filter_images(None)
        if kern is not None:
            ctx.filter_images(kern)
        got = ctx.match_ncc_pyramid_dn(b.xyuvav, b.offset, 16, 7, 3, 2, shift=shift)
        assert ctx.last_path() == PATH[cls]
        return got

    want = []
    for cls, (i0, i1), kern in pairs:
        with api.Context(0) as fresh:
            fresh.set_images(i0, i1)
            want.append(run(fresh, cls, kern))
    with api.Context(0) as ctx:
        prev = None
        for k, (cls, (i0, i1), kern) in enumerate(pairs):
            if prev is None or prev[0] is not i0:
                ctx.set_images(i0, i1)
            got = run(ctx, cls, kern)
            prev = (i0,)
            assert_bits_equal(got[0], want[k][0], f"step {k} ({cls}): record")
            assert_bits_equal(got[1], want[k][1], f"step {k} ({cls}): candidates")
            np.testing.assert_array_equal(got[2], want[k][2], f"step {k} ({cls})")
        ctx.filter_images(None)


@pytest.mark.parametrize("cls", ["u16", "f32"])
def test_device_twin(api, cls):
    from hipmem import DevArray
    c = case(30, 0.03, 8501)
    i0, i1 = as_class(cls, c)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
        d_out, d_cand, d_sho = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32), DevArray((c.n, 2), np.int32)
        # (the first call on the pair: the _dev entry builds the levels itself)
        ctx.match_ncc_pyramid_dn_dev(d_xy.ptr, c.n, c.offset, 30, 8, 3, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, d_shift_out=d_sho.ptr)
        dev, dev_cand, dev_sh = d_out.numpy(), d_cand.numpy(), d_sho.numpy()
        d_out2 = DevArray((c.n, 8), np.float32)
        ctx.match_ncc_pyramid_dn_dev(d_xy.ptr, c.n, c.offset, 30, 8, 3, 0, d_out2.ptr, d_shift=d_sh.ptr)
        dev2 = d_out2.numpy()
        rec, cand, sh = ctx.match_ncc_pyramid_dn(c.xyuvav, c.offset, 30, 8, 3, 4, shift=shift)
    assert_bits_equal(dev, rec, "_dev twin")
    assert_bits_equal(dev_cand, cand, "_dev twin: candidates")
    assert_bits_equal(dev2, rec, "_dev twin without shift_out and candidates")
    np.testing.assert_array_equal(dev_sh, sh)


def test_refusals(api):
    c = case(7, 0.0, 8601)
    i0, i1 = as_class("f32", c)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for ocw, radius, levels in ((7, 0, 2), (7, 16, 2), (8, 5, 2), (7, 5, 0), (7, 5, 6)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), ocw, radius, levels)
            assert e.value.code == -1
        xy = np.ascontiguousarray(c.xyuvav, np.float64)
        out = np.empty((c.n, 8), np.float32)
        cand = np.empty((9, c.n, 3), np.float32)
        sho = np.empty((c.n, 2), np.int32)
        off = np.zeros(2, np.int32)
        call = api._lib.mimc3_match_ncc_pyramid_dn
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 9, 0, out, cand.ctypes.data, sho) == -1         # npeaks 9
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 2, 0, out, None, sho) == -1                     # npeaks without cand
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 0, 0, out, cand.ctypes.data, sho) == -1         # cand without npeaks
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_dn(c.xyuvav, (1 << 25, 0), 7, 5, 2)
        assert e.value.code == -1
        bad = c.xyuvav.copy()
        bad[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_dn(bad, (0, 0), 7, 5, 2)
        assert e.value.code == -2
        rec = ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), 7, 5, 2)[0]                                     # the pair itself is taken ...
        assert ctx.last_path() == "f32i_full"
        with pytest.raises(api.Mimc3Error) as e:                                                         # ... and the older entry refuses it
            ctx.match_ncc_pyramid(c.xyuvav, (0, 0), 7, 5, 2)
        assert e.value.code == -6
        n0 = i0.copy()
        n0[n0 == 0] = np.nan
        n0[5, 5] = np.nan
        ctx.set_images(n0, i1)                                                                           # NaN nulls: a pair of no class
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), 7, 5, 2)
        assert e.value.code == -6
        with pytest.raises(api.Mimc3Error) as e:
            ctx.get_pyramid_level(1)
        assert e.value.code == -6
        ctx.set_images(i0, i1)
        assert_bits_equal(ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), 7, 5, 2)[0], rec, "the pair again, after the refusals")
    # a pair too small for the coarsest level's chip
    t = to_dn16(synth.texture(120, 130, 4), 9)
    with api.Context(0) as ctx:
        ctx.set_images(t, t)
        xy = np.zeros((1, 6))
        xy[0, 2:4] = (60, 60)
        ctx.match_ncc_pyramid_dn(xy, (0, 0), 7, 5, 4)             # level 3 is 15 x 16: it holds a 15-px chip
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_dn(xy, (0, 0), 7, 5, 5)         # level 4 is 7 x 8: it does not
        assert e.value.code == -1
