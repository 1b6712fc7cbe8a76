"""GPU: the exhaustive search with candidates (mimc3_match_ncc_full_multi: the record of mimc3_match_ncc_full plus the best npeaks local
maxima of every point's correlation surface as (du, dv, ncc) candidates) against the test-side oracle (tests/full_multi_oracle.c):
the candidates bit for bit (NaN == NaN), the record bit for bit against Context.match_ncc_full on the same input."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_multi_common import STATUS_R, filled_fraction, full_multi, oracle_postprocess, parity_case, periodic_pair, status_case
from mimc3_amd import synth

pytestmark = pytest.mark.gpu

MX_OCW = (7, 15, 16, 30, 32, 40)
NPEAKS = (1, 3, 8)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.mark.parametrize("radius", [1, 7, 15])
@pytest.mark.parametrize("null_frac", [0.0, 0.03, 0.15])
@pytest.mark.parametrize("ocw", MX_OCW)
def test_parity_every_chip_size_nulls_radius_and_npeaks(api, ocw, null_frac, radius):
    """null_frac 0: the clean form; 0.03 / 0.15: the window-null and general forms too.  npeaks 1, 3 and 8, both directions.  The
    oracle's first npeaks candidates of 8 are its candidates for npeaks (the rank does not depend on how many are asked for)."""
    c, shift = parity_case(ocw, null_frac, radius)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for swap in (False, True):
            sgn = -1 if swap else 1
            off, sh = sgn * c.offset, sgn * shift
            want_out, want = full_multi(c.i0, c.i1, c.xyuvav, off, ocw, radius, 8, shift=sh, swap=swap)
            if radius >= 7:                                     # not vacuous: the slots are filled (the oracle's output)
                assert filled_fraction(want_out, want) >= 0.9
            else:
                assert (want[1:, :, 2] <= -2).all()             # R = 1: one interior cell, at most one candidate
            single = ctx.match_ncc_full(c.xyuvav, off, ocw, radius, shift=sh, swap=swap)
            for npeaks in NPEAKS:
                what = f"ocw {ocw} nulls {null_frac} R {radius} npeaks {npeaks} swap {swap}"
                out, cand = ctx.match_ncc_full_multi(c.xyuvav, off, ocw, radius, npeaks, shift=sh, swap=swap)
                assert ctx.last_path() == "u8_mfma_full"
                assert_bits_equal(out, single, what + ": record vs match_ncc_full")
                assert cand.shape == (npeaks, c.n, 3)
                assert_bits_equal(cand, want[:npeaks], what + ": candidates")
                fit = out[:, 2] >= -1
                assert_bits_equal(cand[0][fit], out[fit, :3], what + ": candidate 0 vs the record")


def test_exact_ties_rank_by_k(api):
    """An exactly periodic pair without nulls (period 6 px on both axes), R 15: offsets a period apart have identical integer sums, so
    bit-equal NCC.  The 25 interior peaks tie; the ranks follow ascending k = (su + R)(2R + 1) + (sv + R)."""
    i0, i1, xy = periodic_pair(6, 6, plateau=False)
    want_out, want, nlm, lmk = full_multi(i0, i1, xy, (0, 0), 15, 15, 8, with_counts=True, lmcap=32)
    S = 31
    ties = [(su + 15) * S + (sv + 15) for su in (-12, -6, 0, 6, 12) for sv in (-12, -6, 0, 6, 12)]
    assert (nlm >= 25).all()
    for g in range(xy.shape[0]):
        assert lmk[g, :25].tolist() == ties                      # the oracle: all 25 equal, in k order
        assert len(set(want[:, g, 2].view(np.uint32).tolist())) == 1
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand = ctx.match_ncc_full_multi(xy, (0, 0), 15, 15, 8)
        assert_bits_equal(out, ctx.match_ncc_full(xy, (0, 0), 15, 15), "record")
    assert_bits_equal(cand, want, "tied candidates")
    cells = np.rint(cand[:, :, :2]).astype(int)
    for g in range(xy.shape[0]):
        assert [(int(a) + 15) * S + int(b) + 15 for a, b in cells[:, g]] == ties[:8]


@pytest.mark.parametrize("radius", [7, 15])
def test_plateau_yields_its_lower_k(api, radius):
    """i1 = B + B moved one row down, B of period 3 on both axes, ocw 7 (a chip and a box of whole periods): NCC(su, sv) ==
    NCC(su, sv + 1) bit for bit wherever sv = 0 mod 3 -- flat tops two cells tall.  Each yields one candidate, its lower k; at R 15
    the top (sv = -15, -14) has its lower cell on the border, so it yields none."""
    i0, i1, xy = periodic_pair(3, 3, plateau=True)
    cap = 128
    want_out, want, nlm, lmk = full_multi(i0, i1, xy, (0, 0), 7, radius, 8, with_counts=True, lmcap=cap)
    S = 2 * radius + 1
    for g in range(xy.shape[0]):
        ks = lmk[g][lmk[g] >= 0]
        su, sv = ks // S - radius, ks % S - radius
        assert len(ks) == nlm[g] and (su % 3 == 0).all() and (sv % 3 == 0).all() and (np.abs(sv) < radius).all()
        assert nlm[g] == len([1 for a in range(-radius + 1, radius) for b in range(-radius + 1, radius) if a % 3 == 0 and b % 3 == 0])
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand = ctx.match_ncc_full_multi(xy, (0, 0), 7, radius, 8)
        assert_bits_equal(out, ctx.match_ncc_full(xy, (0, 0), 7, radius), "record")
    assert_bits_equal(cand, want, "plateau candidates")


def test_slot_statuses(api):
    """-3: every slot (NaN, NaN, -3); -2: every slot (NaN, NaN, -2); -4: the interior local maxima that exist; R = 1: one candidate
    or none; and through the _dev entry a point that breaks the host entry's bounds: the all-NaN record, every slot all NaN."""
    from hipmem import DevArray
    i0, i1, xy = status_case()
    want_out, want = full_multi(i0, i1, xy, (0, 0), 7, STATUS_R, 4)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        out, cand = ctx.match_ncc_full_multi(xy, (0, 0), 7, STATUS_R, 4)
        assert_bits_equal(out, ctx.match_ncc_full(xy, (0, 0), 7, STATUS_R), "record")
        assert_bits_equal(cand, want, "candidates")
        assert out[0, 2] == -3 and (cand[:, 0, 2] == -3).all() and np.isnan(cand[:, 0, :2]).all()
        assert out[1, 2] == -2 and (cand[:, 1, 2] == -2).all() and np.isnan(cand[:, 1, :2]).all()
        assert out[2, 2] == -4 and (cand[:, 2, 2] >= -1).all() and (np.abs(cand[:, 2, :2]) < STATUS_R).all()
        out1, cand1 = ctx.match_ncc_full_multi(xy, (0, 0), 7, 1, 3)
        assert_bits_equal(cand1, full_multi(i0, i1, xy, (0, 0), 7, 1, 3)[1], "R 1")
        assert ((cand1[0, :, 2] >= -1) | (cand1[0, :, 2] <= -2)).all() and (cand1[1:, :, 2] <= -2).all()
        # _dev: point 1's chip leaves the image, point 2's search box leaves the zero border (the host entry refuses both)
        bad = xy.copy()
        bad[1, 2:4] = [3, 60]
        sh = np.zeros((6, 2), np.int32)
        sh[2] = [400, 0]
        d_xy, d_sh, d_out, d_cand = DevArray(src=bad), DevArray(src=sh), DevArray((6, 8), np.float32), DevArray((4, 6, 3), np.float32)
        ctx.match_ncc_full_multi_dev(d_xy.ptr, 6, (0, 0), 7, STATUS_R, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr)
        o, cd = d_out.numpy(), d_cand.numpy()
        assert np.isnan(o[1]).all() and np.isnan(o[2]).all() and np.isnan(cd[:, 1]).all() and np.isnan(cd[:, 2]).all()
        assert_bits_equal(cd[:, [0, 3, 4, 5]], want[:, [0, 3, 4, 5]], "_dev: the other points")
        assert_bits_equal(o[[0, 3, 4, 5]], out[[0, 3, 4, 5]], "_dev: the other records")


def test_refusals(api):
    """npeaks 0 and 9: EINVAL; and every refusal of the single-peak entry: R = 0 and 16, ocw = 8: EINVAL; a chip outside the image, a
    search box beyond the zero border: EBOUNDS; a pair that is not 8-bit: EUNSUPPORTED."""
    c = synth.make_small(seed=21, ocw=7)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for ocw, radius, npeaks in ((7, 5, 0), (7, 5, 9), (7, 5, -1), (7, 0, 2), (7, 16, 2), (8, 5, 2)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full_multi(c.xyuvav, (0, 0), ocw, radius, npeaks)
            assert e.value.code == -1
        xy = c.xyuvav.copy()
        xy[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_multi(xy, (0, 0), 7, 5, 2)
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_multi(c.xyuvav, (300, 0), 7, 5, 2)
        assert e.value.code == -2
        ctx.set_images(c.i0 * 4, c.i1 * 4)
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full_multi(c.xyuvav, (0, 0), 7, 5, 2)
        assert e.value.code == -6


def test_full_size_c2_sample(api):
    """C2 (4096^2, 200,000 points, ocw 16, R 15, centred on the a-priori shift), npeaks 4: the record bit for bit match_ncc_full's,
    the 20,000-point sample of tests/test_full_search.py bit for bit against the oracle; the _dev twin gives the same bytes."""
    from hipmem import DevArray
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        out, cand = ctx.match_ncc_full_multi(c.xyuvav, c.offset, 16, 15, 4, shift=shift)
        single = ctx.match_ncc_full(c.xyuvav, c.offset, 16, 15, shift=shift)
        d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
        d_out, d_cand = DevArray((c.n, 8), np.float32), DevArray((4, c.n, 3), np.float32)
        ctx.match_ncc_full_multi_dev(d_xy.ptr, c.n, c.offset, 16, 15, 4, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr)
        assert_bits_equal(d_out.numpy(), out, "_dev twin: record")
        assert_bits_equal(d_cand.numpy(), cand, "_dev twin: candidates")
    assert_bits_equal(out, single, "record vs match_ncc_full")
    sel = np.random.default_rng(2).choice(c.n, 20000, replace=False)
    sel.sort()
    want_out, want = full_multi(c.i0, c.i1, c.xyuvav[sel], c.offset, 16, 15, 4, shift=shift[sel])
    assert_bits_equal(cand[:, sel], want, "C2 sample: candidates")
    assert_bits_equal(out[sel][:, [0, 1, 2, 3, 5, 6, 7]], want_out[:, [0, 1, 2, 3, 5, 6, 7]], "C2 sample: record")
    fit = out[:, 2] >= -1
    assert fit.mean() > 0.9
    assert_bits_equal(cand[0][fit], out[fit, :3], "candidate 0 vs the record")


def test_join_to_the_post_matcher_chain(api, oracle):
    """GPU candidates of ocw 15, 16, 30 x npeaks 4 stacked pass-major (ndp = 12) through Context.mimc2_postprocess == the oracle's
    candidates through the oracle's chain (cluster_candidates -> dpf0 -> dpf1 -> QM), bit for bit."""
    c = synth.make_small(seed=31, shift=(3, -2), angle_deg=30.0, ocw=16, speed=900.0, h=300, w=320, dimx=12, dimy=10, noise_dn=3,
                         null_frac=0.03, margin=62)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    mps = float(np.float32(c.xyuvav[1, 0] - c.xyuvav[0, 0]))
    gpu, cpu = [], []
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for ocw in (15, 16, 30):
            gpu.append(ctx.match_ncc_full_multi(c.xyuvav, c.offset, ocw, 7, 4, shift=shift)[1])
            cpu.append(full_multi(c.i0, c.i1, c.xyuvav, c.offset, ocw, 7, 4, shift=shift)[1])
        dp_gpu, dp_cpu = np.concatenate(gpu), np.concatenate(cpu)
        assert dp_gpu.shape == (12, c.n, 3)
        assert_bits_equal(dp_gpu, dp_cpu, "stacked candidates")
        got = ctx.mimc2_postprocess(dp_gpu, c.xyuvav, c.dimx, c.dimy, c.dt, c.mpp, mps)
    want = oracle_postprocess(oracle, dp_cpu, c.xyuvav, c.dimx, c.dimy, mps, c.dt, c.mpp)
    assert_bits_equal(got.reshape(5, -1), want, "vxyexyqual")
    ok = ~np.isnan(want[0])
    assert ok.mean() > 0.8
    assert np.abs(want[0][ok] - 3).max() < 0.1 and np.abs(want[1][ok] + 2).max() < 0.1


def test_decoy_recovery(api, oracle):
    """The constructed decoy fixture (full_multi_common.decoy_case; its design is checked on the oracle's chain by
    tests/test_full_multi_oracle.py): GPU candidates through Context.mimc2_postprocess.  npeaks 1: the field is more than 1 px wrong
    at the four decoy points; npeaks 4: within 0.1 px of the truth there.  Candidates and field bit for bit the oracle's."""
    from full_multi_common import DECOY_OCW, DECOY_R, decoy_case, decoy_errors
    c, shift, pts = decoy_case()
    mps = float(np.float32(c.xyuvav[1, 0] - c.xyuvav[0, 0]))
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for npeaks in (1, 4):
            out, cand = ctx.match_ncc_full_multi(c.xyuvav, c.offset, DECOY_OCW, DECOY_R, npeaks, shift=shift)
            want = full_multi(c.i0, c.i1, c.xyuvav, c.offset, DECOY_OCW, DECOY_R, npeaks, shift=shift)[1]
            assert_bits_equal(cand, want, f"decoy candidates, npeaks {npeaks}")
            got = ctx.mimc2_postprocess(cand, c.xyuvav, c.dimx, c.dimy, c.dt, c.mpp, mps).reshape(5, -1)
            assert_bits_equal(got, oracle_postprocess(oracle, want, c.xyuvav, c.dimx, c.dimy, mps, c.dt, c.mpp), f"field, npeaks {npeaks}")
            at, rest = decoy_errors(got, pts)
            print(f"npeaks {npeaks}: error at the decoy points {at.tolist()}, largest elsewhere {rest}")
            assert rest < 0.1
            assert (at > 1.0).all() if npeaks == 1 else (at < 0.1).all()
