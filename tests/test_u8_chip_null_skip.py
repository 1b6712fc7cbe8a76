"""GPU: the chip-null skip of the one-wave 33-pixel 8-bit kernel (match_px_kernel.hip: flag mask, XYC and WNC bodies) on the fixtures of
tests/u8_chip_null_skip_common.py, bit for bit against the port oracle: single chip nulls at every byte phase of a dword column in
either row half, on the tail row (first and last tail lane), in the single valid byte of a row's last dword; a chip that flags all 19
task indices; a disc across the row-16 boundary; window nulls under chip nulls and one pixel off; window bytes 1 / 127 / 128 / 255
under chip nulls; chip nulls with dirty cells on the T4 row and column (the six-sum body must still run there); a chip at the 80 %
rule and one null past it.  Each on a window without nulls (clean boxes: XYC) and with single window nulls (dirty boxes: WNC).
tests/test_u8_chip_null_skip_cpu.py counts that each fixture holds what it is named for.

Paths: the u8 step ("auto": point records, rest list -- the form the skip is switched on for) and the register-tiled kernel alone
("u8px", memory header: it keeps the CHIPNULL / GENERAL bodies, which must give the same bits on the same fixtures)."""
import pytest

import u8_chip_null_skip_common as cn
import u8_dirty_masks_common as dm
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

CASES = [(kind, w) for kind in cn.KINDS for w in cn.WINDOWS] + [(kind, "dirty") for kind in cn.T4_KINDS]


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


@pytest.mark.parametrize("kind,window", CASES)
def test_chip_null_bodies(api, oracle, kind, window):
    c = cn.make_case(kind, window)
    off, uv = dm.pivots(oracle, c)
    want = oracle.match(c.chip_img, c.win_img, c.xyuvav, c.offset, off, uv, c.ocw)
    assert (want[:, 2] != -3).any()
    with api.Context(0) as ctx:
        ctx.set_images(c.chip_img, c.win_img)
        for mode, path in (("u8px", "u8_exact"), ("auto", "u8_mfma")):
            ctx.set_path(mode)
            got = ctx.matching_ncc_dlc_2(c.xyuvav, c.offset, off, uv, c.ocw)
            assert ctx.last_path() == path, (mode, ctx.last_path())
            assert_bits_equal(got, want, f"{kind} {window} {mode}")
