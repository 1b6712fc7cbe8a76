"""GPU: the coarse-to-fine exhaustive search on any f32 pair (mimc3_match_ncc_pyramid_any: float levels, the float kernel per level with
its arg-max cells, the chaining on the device, match_ncc_full_any at level 0).

Exact where exactness exists: the levels equal the numpy reduction bit for bit; record, candidates and shift_out equal, bit for bit,
the chain of match_ncc_full_any(mode 1, surface) calls over the numpy-built levels driven from Python; on integer-class pairs whose
float and integer levels coincide, mode 1 returns the bytes of match_ncc_pyramid_dn.  Against the reference-order oracle
(tests/pyramid_any_oracle.py) shift_out is compared at the points whose coarser-level arg-max the definition determines (the oracle's
best cell leads by more than 2 ulps; tests/test_pyramid_any_oracle.py caps the others at 2 % with the oracle alone)."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import ENCODINGS, float_case
from mimc3_amd import synth
from pyramid_any_oracle import (ORACLE_CASES, ORACLE_LEVELS, ORACLE_R, UNDECIDED_CAP, big_float_case, float_pyr_case, hand_blocks,
                                oracle_case, pyramid_any, pyramid_search_any, upsampled_pair)
from pyramid_dn_oracle import surface_peaks
from pyramid_oracle import BIG, _inside

pytestmark = pytest.mark.gpu

MX_OCW = (7, 15, 16, 30, 32, 40)
PATH = {8: "u8_mfma_full", 12: "u16_full", 16: "f32i_full"}
G = "f32g_full"
R = 6


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_levels(ctx, f0, f1, what, levels=(1, 2, 3)):
    """get_pyramid_level_any against the numpy reduction of the float images f0, f1, bit for bit."""
    p0, p1 = pyramid_any(f0, max(levels) + 1), pyramid_any(f1, max(levels) + 1)
    for lv in levels:
        l0, l1 = ctx.get_pyramid_level_any(lv)
        assert l0.shape == p0[lv].shape and l1.shape == p1[lv].shape
        assert_bits_equal(l0, p0[lv], f"{what}: image 0, level {lv}")
        assert_bits_equal(l1, p1[lv], f"{what}: image 1, level {lv}")


def check_border(ctx, H, W, xyuvav, what):
    """The level planes' borders are zero: every point's level-1 box starts on the first border column right of the level image (so the
    columns a row's last vector wrote are in it) and the level-0 box lies in the border too -- no arg-max on level 1 (d_0 = 2 d_1), -3."""
    ocw, h = 7, 7 + 1
    xy = np.ascontiguousarray(xyuvav, np.float64)
    u0 = xy[:, 2].astype(np.int64)
    d1 = (W >> 1) + h - (u0 >> 1)
    shift = np.stack([2 * d1, np.zeros_like(d1)], axis=1).astype(np.int32)
    rec, _, sh = ctx.match_ncc_pyramid_any(xy, (0, 0), ocw, 1, 2, shift=shift, mode=1)
    assert ctx.last_path() == G
    np.testing.assert_array_equal(sh, shift, what + ": level 1 found an arg-max in the border")
    assert (rec[:, 2] == -3).all(), what + f": statuses {rec[:, 2].tolist()}"


# ---- 1. the reduction alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_levels_of_a_float_pair(api, encoding):
    c, f0, f1, _ = float_case(7, 0.03, R, encoding)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        check_levels(ctx, f0, f1, encoding)
        check_border(ctx, *f0.shape, c.xyuvav, encoding)


def test_levels_of_odd_sizes_filtered_and_8bit_pairs(api):
    c, f0, f1 = float_pyr_case(16, 0.03, 9201, 3, "m9999_nan")
    H, W = f0.shape
    assert H & 1 and W & 1 and (W >> 1) & 1                           # odd sizes on level 0, an odd width on level 1 too
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        check_levels(ctx, f0, f1, "odd sizes")
        check_border(ctx, H, W, c.xyuvav, "odd sizes")
        z0, z1 = np.where(f0 >= 1e-10, f0, 0).astype(np.float32), np.where(f1 >= 1e-10, f1, 0).astype(np.float32)
        ctx.set_images(z0, z1)                                        # (a filter spreads NaN and -9999: zero nulls for this part)
        ctx.filter_images(api.CLI_KERNELS[2])
        g0, g1 = ctx.get_images(H, W)
        assert not np.array_equal(g0, z0) and (g0 != np.rint(g0)).any()
        check_levels(ctx, g0, g1, "filtered: filter, then reduce")
        ctx.filter_images(None)
        check_levels(ctx, z0, z1, "unfiltered again")
        ctx.set_images(c.i0, c.i1)                                    # the 8-bit pair: float levels beside its class
        check_levels(ctx, c.i0, c.i1, "8-bit")
        check_border(ctx, H, W, c.xyuvav, "8-bit")
        assert ctx.get_pyramid_level(1)[0].shape == (H >> 1, W >> 1)  # the integer levels are still served


def test_levels_of_the_hand_built_blocks(api):
    img, want = hand_blocks()
    other = np.ascontiguousarray(img[::-1, ::-1])
    with api.Context(0) as ctx:
        ctx.set_images(img, other)
        check_levels(ctx, img, other, "hand-built", levels=(1, 2))
        l0 = ctx.get_pyramid_level_any(1)[0]
        with np.errstate(over="ignore"):
            assert_bits_equal(l0[0], want.astype(np.float32), "hand-built blocks")
        assert l0[0, 5] == 0 and not np.signbit(l0[0, 5])              # the all-NaN block: the canonical null
        for level in (0, 3, 5):                                       # not a level; 7 >> 3 = 0: empty; beyond 4
            with pytest.raises(api.Mimc3Error) as e:
                ctx.get_pyramid_level_any(level)
            assert e.value.code == -1


# ---- 2. the chain of single-level calls -----------------------------------------------------------------------------------------------
def chain(api, f0, f1, xyuvav, offset, ocw, radius, levels, shift, swap):
    """shift_out as a caller gets it by chaining match_ncc_full_any(mode 1, surface) over the numpy-built levels by hand."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    off = np.asarray(offset, np.int64).reshape(1, 2)
    D = off + (np.zeros((n, 2), np.int64) if shift is None else np.asarray(shift, np.int64))
    uv0 = xy[:, 2:4].astype(np.int64)
    d = D if levels == 1 else (D + (1 << (levels - 2))) >> (levels - 1)
    p0, p1 = pyramid_any(f0, levels), pyramid_any(f1, levels)
    S = 2 * radius + 1
    for lv in range(levels - 1, 0, -1):
        H, W = p0[lv].shape
        pos = uv0 >> lv
        ok = _inside(pos, d, ocw, radius, H, W)                       # (a chip that leaves the level image: no arg-max)
        pk = np.full(n, -1, np.int64)
        if ok.any():
            lxy = np.zeros((int(ok.sum()), 6))
            lxy[:, 2:4] = pos[ok]
            with api.Context(0) as lctx:
                lctx.set_images(p0[lv], p1[lv])
                surf = lctx.match_ncc_full_any(lxy, (0, 0), ocw, radius, 0, shift=d[ok].astype(np.int32), swap=swap, mode=1, surface=True)[2]
            pk[ok] = surface_peaks(surf)
        s = np.where((pk >= 0)[:, None], np.stack([pk // S - radius, pk % S - radius], axis=1), 0)
        d = 2 * (d + s)
    return (d - off).astype(np.int32)


@pytest.mark.parametrize("levels,swap", [(2, False), (3, True)])
@pytest.mark.parametrize("null_frac", [0.0, 0.03])
@pytest.mark.parametrize("ocw", MX_OCW)
def test_chain_identity(api, ocw, null_frac, levels, swap):
    c, f0, f1 = float_pyr_case(ocw, null_frac, 9300 + ocw + int(100 * null_frac) + levels, levels, "nan_zero")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
    what = f"ocw {ocw} nulls {null_frac} L {levels} swap {swap}"
    want_sh = chain(api, f0, f1, c.xyuvav, off, ocw, R, levels, sh_in, swap)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for npeaks in (0, 4):
            rec, cand, sh = ctx.match_ncc_pyramid_any(c.xyuvav, off, ocw, R, levels, npeaks, shift=sh_in, swap=swap)
            assert ctx.last_path() == G
            np.testing.assert_array_equal(sh, want_sh, what)
            full = ctx.match_ncc_full_any(c.xyuvav, off, ocw, R, npeaks, shift=sh, swap=swap)
            assert_bits_equal(rec, full[0], what + f": record vs match_ncc_full_any, npeaks {npeaks}")
            if npeaks:
                assert_bits_equal(cand, full[1], what + ": candidates vs match_ncc_full_any")
            else:
                assert cand is None
        assert (rec[:, 2] >= -1).any() and (sh != sh_in).any()


# ---- 3. against the reference-order oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ocw", ORACLE_CASES)
def test_against_the_reference_order_oracle(api, kind, ocw):
    c, f0, f1, shift = oracle_case(kind, ocw)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for swap in (False, True):
            off, sh_in = (-c.offset, -shift) if swap else (c.offset, shift)
            rec, _, sh = ctx.match_ncc_pyramid_any(c.xyuvav, off, ocw, ORACLE_R, ORACLE_LEVELS, shift=sh_in, swap=swap)
            assert ctx.last_path() == G
            want, _, want_sh, und = pyramid_search_any(f0, f1, c.xyuvav, off, ocw, ORACLE_R, ORACLE_LEVELS, shift=sh_in, swap=swap)
            print(f"{kind} ocw {ocw} swap {swap}: {int(und.sum())} of {c.n} points undecided")
            assert und.mean() <= UNDECIDED_CAP
            np.testing.assert_array_equal(sh[~und], want_sh[~und], f"{kind} ocw {ocw} swap {swap}")
            np.testing.assert_array_equal(rec[~und, 2] == -3, want[~und, 2] == -3)


# ---- 4. mode 1 on the integer classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_mode1_on_integer_pairs_is_match_ncc_pyramid_dn(api, bits):
    i0, i1, xy = upsampled_pair(bits, 9100 + bits)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for levels in (1, 2, 3):
            for swap in (False, True):
                off = (-1, 2) if swap else (1, -2)
                for npeaks in (0, 4):
                    what = f"{bits}-bit L {levels} swap {swap} npeaks {npeaks}"
                    want = ctx.match_ncc_pyramid_dn(xy, off, 7, R, levels, npeaks, swap=swap)
                    assert ctx.last_path() == PATH[bits]
                    for mode, path in ((1, G), (0, PATH[bits])):
                        got = ctx.match_ncc_pyramid_any(xy, off, 7, R, levels, npeaks, swap=swap, mode=mode)
                        assert ctx.last_path() == path
                        np.testing.assert_array_equal(got[2], want[2], what)
                        assert_bits_equal(got[0], want[0], what + f": record, mode {mode}")
                        if npeaks:
                            assert_bits_equal(got[1], want[1], what + f": candidates, mode {mode}")
                        else:
                            assert got[1] is None
                if bits == 8:
                    old, old_sh = ctx.match_ncc_pyramid(xy, off, 7, R, levels, swap=swap)
                    got = ctx.match_ncc_pyramid_any(xy, off, 7, R, levels, swap=swap)
                    np.testing.assert_array_equal(got[2], old_sh)
                    assert_bits_equal(got[0], old, f"L {levels} swap {swap} vs match_ncc_pyramid")
            if levels == 3:
                assert (want[0][:, 2] >= -1).any() and want[2].any()


# ---- 5. large displacement ------------------------------------------------------------------------------------------------------------
def test_large_displacement(api):
    """(+70, -45) px with no prior: three levels recover it wherever the oracle does; one level at R 15 cannot."""
    f0, f1, g = big_float_case()
    du, dv = BIG["motion"]
    ocw = BIG["ocw"]
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        one, _, sh1 = ctx.match_ncc_pyramid_any(g, (0, 0), ocw, 15, 1)
        rec, _, sh = ctx.match_ncc_pyramid_any(g, (0, 0), ocw, 15, 3)
        assert ctx.last_path() == G
    assert not sh1.any()
    want, _, want_sh, und = pyramid_search_any(f0, f1, g, (0, 0), ocw, 15, 3)
    hit = lambda r: (r[:, 2] >= -1) & (np.abs(r[:, 0] - du) < 0.05) & (np.abs(r[:, 1] - dv) < 0.05)
    there = hit(want) & ~und
    assert there.sum() >= 0.9 * ((want[:, 2] >= -1) & ~und).sum() > 0
    assert hit(rec)[there].all()
    np.testing.assert_array_equal(sh[~und], want_sh[~und])
    assert not hit(one)[there].any()                                # status -4 or another peak there


# ---- 6. the remaining cases -----------------------------------------------------------------------------------------------------------
def test_boxes_beyond_the_zero_border(api):
    """Points whose derived level-0 search box leaves the 256-px zero border get the all-NaN record and candidates; no refusal."""
    c, f0, f1 = float_pyr_case(15, 0.0, 9401, 3)
    shift = np.zeros((c.n, 2), np.int32)
    shift[::3] = (400, 0)                              # coarser levels search zeros (-3: no arg-max); level 0's boxes leave the border
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        rec, cand, sh = ctx.match_ncc_pyramid_any(c.xyuvav, (0, 0), 15, 15, 3, 2, shift=shift)
        ok = ctx.match_ncc_pyramid_any(c.xyuvav, (0, 0), 15, 15, 3)[0]        # the context still works
    np.testing.assert_array_equal(sh[::3], shift[::3])
    assert np.isnan(rec[::3]).all() and np.isnan(cand[:, ::3]).all()
    rest = np.ones(c.n, bool)
    rest[::3] = False
    assert not np.isnan(rec[rest, 2]).any() and not np.isnan(cand[0, rest, 2]).any()
    assert (ok[:, 2] >= -1).any()


def test_pair_changes(api):
    """Float, another float, 8-bit in mode 1, mode 0 and mode 1 again, a filtered float pair and back on one context: both level sets
    follow the pair, and every result is a fresh context's."""
    a = float_pyr_case(16, 0.03, 9501, 3)
    b = float_pyr_case(16, 0.03, 9502, 3, "nan_zero")
    c = b[0]
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    zb = (np.nan_to_num(b[1], nan=0.0), b[2])
    lap = api.CLI_KERNELS[2]
    steps = [((a[1], a[2]), None, 0, G), ((b[1], b[2]), None, 0, G), ((c.i0, c.i1), None, 1, G), ((c.i0, c.i1), None, 0, "u8_mfma_full"),
             ((c.i0, c.i1), None, 1, G), (zb, lap, 0, G), (zb, None, 0, G), ((c.i0, c.i1), lap, 1, G), ((c.i0, c.i1), lap, 0, "u16_full")]

    def run(ctx, kern, mode, path):
        ctx.filter_images(None)
        if kern is not None:
            ctx.filter_images(kern)
        got = ctx.match_ncc_pyramid_any(c.xyuvav, c.offset, 16, 7, 3, 2, shift=shift, mode=mode)
        assert ctx.last_path() == path
        return got

    want = []
    for (i0, i1), kern, mode, path in steps:
        with api.Context(0) as fresh:
            fresh.set_images(i0, i1)
            want.append(run(fresh, kern, mode, path))
    assert not np.array_equal(want[5][2], want[6][2]) or not np.array_equal(want[5][0], want[6][0], equal_nan=True)
    with api.Context(0) as ctx:
        prev = None
        for k, ((i0, i1), kern, mode, path) in enumerate(steps):
            if prev is not i0:
                ctx.set_images(i0, i1)
            prev = i0
            got = run(ctx, kern, mode, path)
            assert_bits_equal(got[0], want[k][0], f"step {k}: record")
            assert_bits_equal(got[1], want[k][1], f"step {k}: candidates")
            np.testing.assert_array_equal(got[2], want[k][2], f"step {k}")
        ctx.filter_images(None)


def test_device_twin(api):
    import ctypes as C
    import hipmem
    from hipmem import DevArray
    c, f0, f1 = float_pyr_case(30, 0.03, 9601, 3, "m9999_nan")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
        d_out, d_cand, d_sho = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32), DevArray((c.n, 2), np.int32)
        st = C.c_void_p()                                       # a caller's stream, of the runtime the library runs on
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        # (the first call on the pair: the _dev entry builds the planes and the levels itself)
        ctx.match_ncc_pyramid_any_dev(d_xy.ptr, c.n, c.offset, 30, 8, 3, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, d_shift_out=d_sho.ptr,
                                      stream=st.value)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        dev, dev_cand, dev_sh = d_out.numpy(), d_cand.numpy(), d_sho.numpy()
        d_out2 = DevArray((c.n, 8), np.float32)
        ctx.match_ncc_pyramid_any_dev(d_xy.ptr, c.n, c.offset, 30, 8, 3, 0, d_out2.ptr, d_shift=d_sh.ptr, stream=st.value, mode=1)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        dev2 = d_out2.numpy()
        assert ctx.last_path() == G
        rec, cand, sh = ctx.match_ncc_pyramid_any(c.xyuvav, c.offset, 30, 8, 3, 4, shift=shift)
        rec0 = ctx.match_ncc_pyramid_any(c.xyuvav, c.offset, 30, 8, 3, 0, shift=shift)[0]
        assert hipmem._hip.hipStreamDestroy(st) == 0
    assert_bits_equal(dev, rec, "_dev twin")
    assert_bits_equal(dev_cand, cand, "_dev twin: candidates")
    assert_bits_equal(dev2, rec0, "_dev twin without shift_out and candidates")
    np.testing.assert_array_equal(dev_sh, sh)
    assert (rec[:, 2] >= -1).any()


def test_refusals(api):
    c, f0, f1 = float_pyr_case(7, 0.0, 9701, 3, "nan_zero")
    f0[5, 5] = np.nan
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        for ocw, radius, levels in ((7, 0, 2), (7, 16, 2), (8, 5, 2), (7, 5, 0), (7, 5, 6)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_pyramid_any(c.xyuvav, (0, 0), ocw, radius, levels)
            assert e.value.code == -1
        for mode in (-1, 2):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_pyramid_any(c.xyuvav, (0, 0), 7, 5, 2, mode=mode)
            assert e.value.code == -1
        xy = np.ascontiguousarray(c.xyuvav, np.float64)
        out = np.empty((c.n, 8), np.float32)
        cand = np.empty((9, c.n, 3), np.float32)
        sho = np.empty((c.n, 2), np.int32)
        off = np.zeros(2, np.int32)
        call = api._lib.mimc3_match_ncc_pyramid_any
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 9, 0, 0, out, cand.ctypes.data, sho) == -1      # npeaks 9
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 2, 0, 0, out, None, sho) == -1                  # npeaks without cand
        assert call(ctx._h, xy, c.n, off, None, 7, 5, 2, 0, 0, 0, out, cand.ctypes.data, sho) == -1      # cand without npeaks
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_any(c.xyuvav, (1 << 25, 0), 7, 5, 2)
        assert e.value.code == -1
        bad = c.xyuvav.copy()
        bad[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_any(bad, (0, 0), 7, 5, 2)
        assert e.value.code == -2
        rec = ctx.match_ncc_pyramid_any(c.xyuvav, (0, 0), 7, 5, 2)[0]                                    # the pair itself is taken ...
        assert ctx.last_path() == G
        with pytest.raises(api.Mimc3Error) as e:                                                         # ... and the older entries refuse it
            ctx.match_ncc_pyramid_dn(c.xyuvav, (0, 0), 7, 5, 2)
        assert e.value.code == -6
        with pytest.raises(api.Mimc3Error) as e:
            ctx.get_pyramid_level(1)
        assert e.value.code == -6
        assert_bits_equal(ctx.match_ncc_pyramid_any(c.xyuvav, (0, 0), 7, 5, 2)[0], rec, "the pair again, after the refusals")
    # a pair too small for the coarsest level's chip
    t = np.ascontiguousarray(synth.texture(120, 130, 4) * np.float32(0.37))
    with api.Context(0) as ctx:
        ctx.set_images(t, t)
        xy = np.zeros((1, 6))
        xy[0, 2:4] = (60, 60)
        ctx.match_ncc_pyramid_any(xy, (0, 0), 7, 5, 4)            # level 3 is 15 x 16: it holds a 15-px chip
        assert ctx.last_path() == G
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_pyramid_any(xy, (0, 0), 7, 5, 5)        # level 4 is 7 x 8: it does not
        assert e.value.code == -1
