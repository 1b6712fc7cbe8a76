"""GPU: the exhaustive search beyond +-15 px (mimc3_match_ncc_wide, match_wide_kernel.hip).

Every comparison is against the CPU oracle (tests/full_any_oracle.c: full_any and tail_from_surface; tests/test_wide_cpu.py shows that it
is the definition at large R), never against another run of the new kernel:
  * surface   bit for bit on 8-bit and 16-bit pairs, whose sums are exact in any order; on float pairs the same finite mask and every
              finite cell within 1 f32 ulp -- the margin tests/test_full_any.py grants the float kernel, for the same reason (the order
              of the f64 additions is the kernel's own, additions only, (m - 1) 2^-53 with m <= 6,561 whatever R is);
  * record and candidates (K = 8)   the oracle's tail of the DEVICE surface, bit for bit on all 8 columns (SNR in the device's order);
  * R <= 15 is mimc3_match_ncc_full_any(mode 1) byte for byte; the central block of an R-16 surface is the R-15 surface."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import float_case, full_any, surface_distance, tail_from_surface, to_float
from full_multi_common import periodic_pair
from mimc3_amd import synth
from wide_common import (CASES, CRAFT_OCW, CRAFT_R, CRAFT_PERIOD, FAR_OCW, FAR_R, FAR_TRUE, MAX_RADIUS, case_id, far_case, fixture, oracle)

pytestmark = pytest.mark.gpu

K = 8
WIDE, FULL = "f32g_wide", "f32g_full"


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def check_against_oracle(ctx, i0, i1, xy, off, ocw, R, shift, swap, exact, what, want=None):
    """Surface against the oracle (bit for bit / within 1 ulp), then record and candidates against the oracle's tail of the device
    surface -> (record, candidates, surface)"""
    want_rec, want_surf = want if want is not None else full_any(i0, i1, xy, off, ocw, R, 0, shift=shift, swap=swap)[0:3:2]
    rec, cand, surf = ctx.match_ncc_wide(xy, off, ocw, R, K, shift=shift, swap=swap, surface=True)
    assert ctx.last_path() == (WIDE if R >= 16 else FULL)
    st3 = want_rec[:, 2] == -3
    assert np.array_equal(rec[:, 2] == -3, st3), what + ": status -3 points"
    assert np.isnan(surf[st3]).all()
    if exact:
        assert_bits_equal(surf, want_surf, what + ": surface vs the oracle")
    else:
        share, worst = surface_distance(surf, want_surf, what)
        print(f"{what}: {share:.6f} of the finite cells differ from the oracle, at most {worst} ulp")
        assert worst <= 1, f"{what}: a cell {worst} ulp from the oracle"
    t_rec, t_cand = tail_from_surface(surf, shift, R, K, refused=st3, device_snr_order=True)
    assert_bits_equal(rec, t_rec, what + ": record vs the tail of the device surface")
    assert_bits_equal(cand, t_cand, what + ": candidates vs the tail of the device surface")
    rec0, none = ctx.match_ncc_wide(xy, off, ocw, R, 0, shift=shift, swap=swap)
    assert none is None
    assert_bits_equal(rec0, t_rec, what + ": the record alone")
    return rec, cand, surf


# ---- 1, 2. surface, record and candidates ----
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_surface_record_candidates(api, case):
    f = fixture(case)
    assert f["R"] <= api.wide_max_radius(f["ocw"])
    with api.Context(0) as ctx:
        ctx.set_images(f["i0"], f["i1"])
        rec, cand, surf = check_against_oracle(ctx, f["i0"], f["i1"], f["xy"], f["off"], f["ocw"], f["R"], f["shift"], f["swap"],
                                               f["exact"], f["what"], want=oracle(case)[:2])
    assert np.isfinite(rec[:, 0]).any() and rec[f["g4"], 2] == -4 and rec[f["g3"], 2] == -3
    assert (cand[:, f["g4"], 2] >= -1).all(), "status -4: the interior candidates are listed"
    assert (cand[:, f["g3"], 2] == -3).all()
    if f["g3box"] is not None:                              # the box rule: a valid chip in a box that is null throughout
        assert rec[f["g3box"], 2] == -3 and (cand[:, f["g3box"], 2] == -3).all() and np.isnan(surf[f["g3box"]]).all()


def test_crafted_ties_and_border_peak(api):
    """More than 8 local maxima, the best nine exactly tied (a period apart), and the first-wins arg-max on the border; and the plateau
    form of the same pair."""
    for plateau in (False, True):
        p0, p1, xy = periodic_pair(*CRAFT_PERIOD, plateau=plateau)
        with api.Context(0) as ctx:
            ctx.set_images(p0, p1)
            rec, cand, surf = check_against_oracle(ctx, p0, p1, xy, (0, 0), CRAFT_OCW, CRAFT_R, None, False, True, f"periodic, plateau {plateau}")
        if not plateau:
            assert (rec[:, 2] == -4).all() and np.isfinite(cand).all() and (cand[:, :, 2] == cand[0, :, 2]).all()


# ---- 3. hand-over at R <= 15 ----
@pytest.mark.parametrize("as_float", [False, True])
def test_r15_is_full_any(api, as_float):
    c, f0, f1, shift = float_case(16, 0.03, 15, "nan_zero")
    i0, i1 = (f0, f1) if as_float else (c.i0, c.i1)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        for npeaks in (0, 4):
            want = ctx.match_ncc_full_any(c.xyuvav, c.offset, 16, 15, npeaks, shift=shift, mode=1, surface=True)
            got = ctx.match_ncc_wide(c.xyuvav, c.offset, 16, 15, npeaks, shift=shift, surface=True)
            assert ctx.last_path() == FULL
            for a, b, name in zip(got, want, ("record", "candidates", "surface")):
                if b is None:
                    assert a is None
                else:
                    assert a.tobytes() == b.tobytes(), f"R 15, npeaks {npeaks}: {name}"


# ---- 4. continuity across the two kernels ----
@pytest.mark.parametrize("as_float", [False, True])
def test_r16_continues_r15(api, as_float):
    c, f0, f1, shift = float_case(7, 0.03, 16, "zero")
    i0, i1 = (f0, f1) if as_float else (c.i0, c.i1)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        r15, _, s15 = ctx.match_ncc_full_any(c.xyuvav, c.offset, 7, 15, 0, shift=shift, mode=1, surface=True)
        assert ctx.last_path() == FULL
        r16, _, s16 = ctx.match_ncc_wide(c.xyuvav, c.offset, 7, 16, 0, shift=shift, surface=True)
        assert ctx.last_path() == WIDE
    both = (r15[:, 2] != -3) & (r16[:, 2] != -3)
    assert both.sum() >= 12
    block = s16.reshape(-1, 33, 33)[:, 1:32, 1:32].reshape(-1, 31 * 31)
    if as_float:
        share, worst = surface_distance(block[both], s15[both], "R 16 vs R 15, float")
        print(f"float: {share:.6f} of the cells differ between the two kernels, at most {worst} ulp")
        assert worst <= 2                                   # each side is within 1 of the oracle
    else:
        assert_bits_equal(block[both], s15[both], "central 31 x 31 block of the R-16 surface vs the R-15 surface")


# ---- 5. what it is for ----
def test_displacement_beyond_15_px(api):
    c = far_case()
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        far, _ = ctx.match_ncc_wide(c.xyuvav, (0, 0), FAR_OCW, FAR_R, 0)
        assert ctx.last_path() == WIDE
        near, _ = ctx.match_ncc_full_any(c.xyuvav, (0, 0), FAR_OCW, 15, 0)
    fitted = np.isfinite(far[:, 0])
    assert fitted.all()                                     # (the oracle fits every point: tests/test_wide_cpu.py)
    assert np.hypot(far[fitted, 0] - FAR_TRUE[0], far[fitted, 1] - FAR_TRUE[1]).max() < 0.5
    nf = np.isfinite(near[:, 0])
    assert (np.hypot(near[nf, 0] - FAR_TRUE[0], near[nf, 1] - FAR_TRUE[1]) > 15).all()


# ---- 6. refusals ----
def test_refusals_and_max_radius(api):
    assert api.wide_max_radius(8) == 0 and api.wide_max_radius(0) == 0
    for ocw in (7, 15, 16):
        assert api.wide_max_radius(ocw) >= 47
    assert api.wide_max_radius(40) >= 31
    assert {ocw: api.wide_max_radius(ocw) for ocw in MAX_RADIUS} == MAX_RADIUS
    c = synth.make_small(seed=21, ocw=7)
    f0, f1 = to_float(c.i0, 1), to_float(c.i1, 2)
    xy = np.ascontiguousarray(c.xyuvav, np.float64)
    out = np.empty((c.n, 8), np.float32)
    cand = np.empty((9, c.n, 3), np.float32)
    off = np.zeros(2, np.int32)
    call = api._lib.mimc3_match_ncc_wide
    with api.Context(0) as ctx:
        assert call(ctx._h, xy, c.n, off, None, 7, 20, 0, 0, out, None, None) == -5                   # no images: MIMC3_ESTATE
        ctx.set_images(f0, f1)
        assert call(ctx._h, xy, c.n, off, None, 7, 20, 9, 0, out, cand.ctypes.data, None) == -1       # npeaks 9
        assert call(ctx._h, xy, c.n, off, None, 7, 20, 2, 0, out, None, None) == -1                   # cand / npeaks mismatch
        assert call(ctx._h, xy, c.n, off, None, 7, 20, 0, 0, out, cand.ctypes.data, None) == -1
        for ocw, radius in ((7, 0), (7, api.wide_max_radius(7) + 1), (40, api.wide_max_radius(40) + 1), (8, 20)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_wide(c.xyuvav, (0, 0), ocw, radius, 2)
            assert e.value.code == -1
        bad = c.xyuvav.copy()
        bad[3, 2] = 3.0                                                                                # a chip outside the image
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_wide(bad, (0, 0), 7, 20, 2)
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_wide(c.xyuvav, (300, 0), 7, 20, 2)                                           # a box outside the zero border
        assert e.value.code == -2
        rec, _ = ctx.match_ncc_wide(c.xyuvav, (0, 0), 7, 16, 0)
        assert ctx.last_path() == WIDE
        ctx.match_ncc_wide(c.xyuvav, (0, 0), 7, 15, 0)
        assert ctx.last_path() == FULL
        for entry in (ctx.match_ncc_full_any, ctx.match_ncc_full_fb):                                   # the older entries keep their range
            with pytest.raises(api.Mimc3Error) as e:
                entry(c.xyuvav, (0, 0), 7, 16, 0)
            assert e.value.code == -1
        assert_bits_equal(ctx.match_ncc_wide(c.xyuvav, (0, 0), 7, 16, 0)[0], rec, "the pair again, after the refusals")


# ---- 7. the _dev entry ----
def test_dev_entry(api):
    import hipmem
    from hipmem import DevArray
    c, f0, f1, shift = float_case(16, 0.03, 20, "nan_zero")
    R, ocw = 20, 16
    S2 = (2 * R + 1) ** 2
    xy = np.ascontiguousarray(c.xyuvav).copy()
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        out, cand, surf = ctx.match_ncc_wide(xy, c.offset, ocw, R, 4, shift=shift, surface=True)
        xy_bad = xy.copy()
        xy_bad[2, 2] = 5.0                                  # the chip leaves the image: only the _dev entry can be handed such a point
        d_xy, d_sh = DevArray(src=xy_bad), DevArray(src=np.ascontiguousarray(shift, np.int32))
        d_out, d_cand, d_surf = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32), DevArray((c.n, S2), np.float32)
        st = C.c_void_p()
        assert hipmem._hip.hipStreamCreate(C.byref(st)) == 0 and st.value
        ctx.match_ncc_wide_dev(d_xy.ptr, c.n, c.offset, ocw, R, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr, stream=st.value, d_surf=d_surf.ptr)
        assert hipmem._hip.hipStreamSynchronize(st) == 0
        assert ctx.last_path() == WIDE
        g_out, g_cand, g_surf = d_out.numpy(), d_cand.numpy(), d_surf.numpy()
        assert hipmem._hip.hipStreamDestroy(st) == 0
    ok = np.arange(c.n) != 2
    assert g_out[ok].tobytes() == out[ok].tobytes() and g_cand[:, ok].tobytes() == cand[:, ok].tobytes()
    assert g_surf[ok].tobytes() == surf[ok].tobytes()
    assert np.isnan(g_out[2]).all() and np.isnan(g_surf[2]).all() and np.isnan(g_cand[:, 2]).all()
