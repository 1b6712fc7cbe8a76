"""GPU: the exhaustive-search entry (mimc3_match_ncc_full: every (2R + 1)^2 cell of a point on the matrix cores, with the peak-quality
record) against the test-side oracle (tests/full_search_oracle.c): every column bit for bit but the SNR (column 4, an f64 sum in
another order), which is within 1 f32 ulp."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_search_common import assert_records_match, full_search
from mimc3_amd import synth

pytestmark = pytest.mark.gpu

MX_OCW = (7, 15, 16, 30, 32, 40)


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.mark.parametrize("radius", [1, 7, 15])
@pytest.mark.parametrize("null_frac", [0.0, 0.03, 0.15])
@pytest.mark.parametrize("ocw", MX_OCW)
def test_every_chip_size_nulls_and_radius(api, ocw, null_frac, radius):
    """null_frac 0: the clean form; 0.03 / 0.15: points with window nulls (window-null form) and chip nulls (general form) too.
    Both directions; the a-priori shift centres the searches."""
    c = synth.make_small(seed=7100 + ocw + int(100 * null_frac) + radius, shift=(3, -2), angle_deg=40.0, ocw=ocw, speed=700.0,
                         h=2 * ocw + 200, w=2 * ocw + 210, dimx=6, dimy=5, noise_dn=2, null_frac=null_frac, offset=(1, -1))
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        got = ctx.match_ncc_full(c.xyuvav, c.offset, ocw, radius, shift=shift)
        assert ctx.last_path() == "u8_mfma_full"
        assert_records_match(got, full_search(c.i0, c.i1, c.xyuvav, c.offset, ocw, radius, shift=shift), f"ocw {ocw} nulls {null_frac} R {radius}")
        sw = ctx.match_ncc_full(c.xyuvav, -c.offset, ocw, radius, shift=-shift, swap=True)
        assert_records_match(sw, full_search(c.i0, c.i1, c.xyuvav, -c.offset, ocw, radius, shift=-shift, swap=True),
                             f"ocw {ocw} nulls {null_frac} R {radius} swapped")


def test_status_edge_cases(api):
    """-3: a search box more than 80 % null; -2: a flat chip (every cell 0 / 0); -4: the peak on the border; and points whose boxes
    overhang the image edge (the zero border: nulls)."""
    H = W = 128
    i0 = synth.texture(H, W, 3, sigma=3.0)                    # smooth: the NCC climbs toward the true offset
    i1 = np.roll(i0, (0, 5), axis=(0, 1)).copy()
    i1[10:70, 10:70] = 0                                       # point 0's box: > 80 % null
    i0[80 - 7:80 + 8, 40 - 7:40 + 8] = 9                       # point 1's chip: flat
    xy = np.zeros((6, 6))
    xy[:, 2:4] = [[40, 40], [40, 80], [90, 90], [7, 60], [120, 120], [60, 7]]   # 2: true offset +5 > R = 3; 3-5: boxes over the edge
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        got = ctx.match_ncc_full(xy, (0, 0), 7, 3)
        assert_records_match(got, full_search(i0, i1, xy, (0, 0), 7, 3), "edge cases")
        assert got[0, 2] == -3 and got[1, 2] == -2 and got[2, 2] == -4
        assert np.isnan(got[:3, [0, 1, 3, 4, 5, 6, 7]]).all()
        got = ctx.match_ncc_full(xy, (0, 0), 7, 15)
        assert_records_match(got, full_search(i0, i1, xy, (0, 0), 7, 15), "edge cases R 15")
        assert got[2, 2] > 0.99 and abs(got[2, 0] - 5) < 0.05


def test_shift_equals_a_moved_pair(api):
    """shift = k on a pair whose i1 is moved by k: the record of shift = 0 on the unmoved pair (columns 2-7 bit for bit; du, dv carry
    k), and both equal to the oracle."""
    c = synth.make_small(seed=17, shift=(2, 1), ocw=15, h=230, w=240, null_frac=0.03, noise_dn=2)
    k = np.array([4, -3])
    i1m = np.zeros_like(c.i1)
    Hh, Ww = c.i1.shape
    i1m[max(k[1], 0):Hh + min(k[1], 0), max(k[0], 0):Ww + min(k[0], 0)] = c.i1[max(-k[1], 0):Hh + min(-k[1], 0), max(-k[0], 0):Ww + min(-k[0], 0)]
    sh = np.tile(k, (c.n, 1)).astype(np.int32)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        base = ctx.match_ncc_full(c.xyuvav, (0, 0), 15, 6)
        ctx.set_images(c.i0, i1m)
        moved = ctx.match_ncc_full(c.xyuvav, (0, 0), 15, 6, shift=sh)
    assert_records_match(moved, full_search(c.i0, i1m, c.xyuvav, (0, 0), 15, 6, shift=sh), "moved pair")
    good = base[:, 2] >= -1
    assert good.sum() > c.n // 2
    assert_bits_equal(moved[:, 2:], base[:, 2:], "k vs 0")
    assert np.allclose(moved[good, :2] - k, base[good, :2], rtol=0, atol=1e-5)


def test_refusals(api):
    """R = 0 and 16, ocw = 8: EINVAL; a chip outside the image: EBOUNDS; a pair that is not 8-bit: EUNSUPPORTED."""
    c = synth.make_small(seed=21, ocw=7)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        for ocw, radius in ((7, 0), (7, 16), (8, 5)):
            with pytest.raises(api.Mimc3Error) as e:
                ctx.match_ncc_full(c.xyuvav, (0, 0), ocw, radius)
            assert e.value.code == -1
        xy = c.xyuvav.copy()
        xy[3, 2] = 3.0
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full(xy, (0, 0), 7, 5)
        assert e.value.code == -2
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full(c.xyuvav, (300, 0), 7, 5)             # the search box beyond the 256-px zero border
        assert e.value.code == -2
        ctx.set_images(c.i0 * 4, c.i1 * 4)                          # 10-bit values: the u16 planes
        with pytest.raises(api.Mimc3Error) as e:
            ctx.match_ncc_full(c.xyuvav, (0, 0), 7, 5)
        assert e.value.code == -6


@pytest.mark.parametrize("seed", [7, 11])
def test_known_motion(api, seed):
    """On make_small(shift=(3, -2)) -- the smoke test's pair, at a matrix-core chip size -- every valid point recovers the pair's
    displacement (offset + du, dv) to within 0.05 px, as the DLC matcher does on the same pair."""
    c = synth.make_small(seed=seed, shift=(3, -2), angle_deg=30.0, ocw=16, noise_dn=2, null_frac=0.03)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        got = ctx.match_ncc_full(c.xyuvav, c.offset, 16, 7, shift=api.prior_shift(c.xyuvav, c.dt, c.mpp))
    ok = got[:, 2] >= -1
    assert ok.sum() >= 0.9 * c.n
    assert np.abs(got[ok, 0] + c.offset[0] - 3).max() < 0.05 and np.abs(got[ok, 1] + c.offset[1] + 2).max() < 0.05


def test_full_size_c2_sample(api):
    """C2 (4096^2, 200,000 points, ocw 16, R 15, centred on the a-priori shift): the whole pass on the device, a 20,000-point sample
    bit for bit against the oracle; the _dev twin gives the same bytes."""
    from hipmem import DevArray
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        got = ctx.match_ncc_full(c.xyuvav, c.offset, 16, 15, shift=shift)
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        ctx.match_ncc_full_dev(d_xy.ptr, c.n, c.offset, 16, 15, d_out.ptr, d_shift=d_sh.ptr)
        dev = d_out.numpy()
    assert_bits_equal(dev, got, "_dev twin")
    sel = np.random.default_rng(2).choice(c.n, 20000, replace=False)
    sel.sort()
    assert_records_match(got[sel], full_search(c.i0, c.i1, c.xyuvav[sel], c.offset, 16, 15, shift=shift[sel]), "C2 sample")
    assert (got[:, 2] >= -1).mean() > 0.9
