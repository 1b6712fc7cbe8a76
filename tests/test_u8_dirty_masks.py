"""GPU: the masked bodies of the register-tiled 8-bit kernels (window-null cells: three sums + table, six sums on a T4 round, six
sums with chip-derived masks) on the fixtures of tests/u8_dirty_masks_common.py, bit for bit against the port oracle: single nulls at
every byte phase of window and box, nulls under pad bytes and one pixel outside a box, neighbours 1 / 127 / 128 / 255 of a null, a
blob edge through the climb area, dirty cells on the T4 row and column, nulls in chip and window, a box with one valid pixel in a
search area one pixel short of the 80 % rule.  tests/test_u8_dirty_masks_cpu.py counts that each fixture holds what it is named for.

Paths: the register-tiled kernel alone ("u8px"), the u8 step ("auto": the classifier sends window-null points down the rest list),
the per-point offset policy on the same geometry lifted to 9 bits, and on a filtered (d/dx) pair."""
import numpy as np
import pytest

import u8_dirty_masks_common as dm
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

DDX = np.array([[-1, 0, 1]], np.float32)
CASES = [(ocw, kind) for ocw in (7, 16) for kind in dm.KINDS]
BIG = [(40, "t4_row", 0), (40, "t4_col", 200)]           # four waves per point: the six-sum body parks through LDS atomics


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def run(api, oracle, c, modes, paths, what):
    off, uv = dm.pivots(oracle, c)
    want = oracle.match(c.chip_img, c.win_img, c.xyuvav, c.offset, off, uv, c.ocw)
    assert (want[:, 2] != -3).any()
    with api.Context(0) as ctx:
        ctx.set_images(c.chip_img, c.win_img)
        for mode in modes:
            ctx.set_path(mode)
            got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, c.ocw)
            assert ctx.last_path() in paths[mode], (mode, ctx.last_path())
            assert_bits_equal(got, want, f"{what} {mode}")


@pytest.mark.parametrize("ocw,kind", CASES)
def test_window_null_bodies_u8(api, oracle, ocw, kind):
    run(api, oracle, dm.make_case(ocw, kind), ("u8px", "auto"), {"u8px": ("u8_exact",), "auto": ("u8_mfma",)}, f"ocw {ocw} {kind}")


@pytest.mark.parametrize("ocw,kind", CASES)
def test_window_null_bodies_offset_policy(api, oracle, ocw, kind):
    """The same geometry with every valid pixel lifted by 200: no longer 8-bit, every local range fits a byte."""
    run(api, oracle, dm.make_case(ocw, kind, lift=200), ("auto", "u8px"), {"auto": ("u8_offset",), "u8px": ("u8_offset",)}, f"ocw {ocw} {kind} + 200")


@pytest.mark.parametrize("ocw,kind,lift", BIG)
def test_window_null_bodies_four_waves(api, oracle, ocw, kind, lift):
    paths = {"u8px": ("u8_offset",) if lift else ("u8_exact",), "auto": ("u8_offset",) if lift else ("u8_mfma",)}
    run(api, oracle, dm.make_case(ocw, kind, lift), ("u8px", "auto"), paths, f"ocw {ocw} {kind} + {lift}")


@pytest.mark.parametrize("ocw,kind", [(7, "carry"), (16, "blob_edge"), (16, "both_sides"), (16, "t4_row")])
def test_window_null_bodies_filtered_pair(api, oracle, ocw, kind):
    """d/dx of the 8-bit fixture (9-bit integers; a null spreads over its row neighbours): filtered on the device, matched there, against
    the oracle's filter and matcher."""
    c = dm.make_case(ocw, kind)
    off, uv = dm.pivots(oracle, c)
    f0, f1 = oracle.float_conv2(c.chip_img, DDX), oracle.float_conv2(c.win_img, DDX)
    want = oracle.match(f0, f1, c.xyuvav, c.offset, off, uv, ocw)
    with api.Context(0) as ctx:
        ctx.set_images(c.chip_img, c.win_img)
        ctx.filter_images(DDX)
        got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, ocw)
        assert ctx.last_path() in ("u8_offset", "u16_scaled", "u8_mfma"), ctx.last_path()       # (small gradients can still be 8-bit)
    assert_bits_equal(got, want, f"ocw {ocw} {kind} d/dx")
    assert (want[:, 2] != -3).any() and (dm.MaskCase(kind, ocw, f0, f1, c.xyuvav, c.offset, c.x0, c.y0).window(0)[:-1, :-1] == 0).any()
