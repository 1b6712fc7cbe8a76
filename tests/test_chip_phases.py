"""GPU: the run-time-ocw matrix-core searches -- match_ncc_full_chip_class ("u8_mfma_chip"), match_ncc_full_chip_planes ("u16_mfma_chip"),
match_ncc_wide_class beyond +-15 px ("u8_mfma_wide") and match_ncc_wide_planes beyond +-15 px ("u16_mfma_wide") -- at every pixel phase of chip and window origin with every null class, with
one null at every position that a byte mask or a chunk boundary can get wrong, with search boxes at the end of the zero-bordered plane
and at fractional coordinates.

The fixtures and call lists are those of tests/chip_phase_common.py, qualified without a device by tests/test_chip_phases_cpu.py.  The
judge is the CPU oracle of tests/full_any_common.py, compared as tests/test_wide_u8.py compares: the surface bit for bit (a non-finite
cell of the same kind), record and candidates the oracle's tail of the device surface and of the oracle surface, the statuses -2, -3, -4
point for point; no tolerance.  Every call runs in mode 1 and asserts last_path(), so that no fallback stands in for the kernel under
test; every call runs at npeaks 0 and 4, with surfaces and without."""
import numpy as np
import pytest

import chip_phase_common as cp
from conftest import assert_bits_equal
from phase_common import fractional, plane_end_points, search_shifts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


# ---- 1. every phase pair with every null class ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,part", cp.PHASE_PARTS, ids=[f"{cp.case_id(c)}-{p}" for c, p in cp.PHASE_PARTS])
def test_every_phase_with_every_null_class(api, case, part):
    """the 64 points of the phase fixture at the four offsets in u: with the a-priori shift, without it, and two calls swapped"""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for k in cp.part_calls(part):
            offset, shift, swap = calls[k]
            o_rec, o_surf = cp.phase_oracle(case, k)
            cp.check_call(ctx, entry, f, f.xy, radius, offset, shift, swap, o_rec, o_surf,
                          f"{cp.case_id(case)}, offset {offset.tolist()}, shift {shift is not None}, swap {swap}")


# ---- 2. one null per point ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cp.SWEEP_CASES, ids=[cp.case_id(c) for c in cp.SWEEP_CASES])
def test_one_null_at_every_mask_and_chunk_boundary(api, case):
    """all points in one launch: chip nulls in every byte lane of the first dword, on both sides of the K chunks of a chip row and under
    the LASTN mask; box nulls likewise and on both sides of the 64-row chunks of the vertical sums; in the wide kernel on both sides of
    every tile window's first and last pixel, where the per-tile query decides whether the null corrections run"""
    entry, kind, ocw, radius = case
    fx = cp.sweep_fixture(case)
    o_rec, o_surf = cp.sweep_oracle(fx)
    with api.Context(0) as ctx:
        ctx.set_images(fx.i0, fx.i1)
        got = cp.check_call(ctx, entry, fx, fx.xy, radius, fx.offset, fx.shift, False, o_rec, o_surf, cp.case_id(case))
    rec, _, surf = got[0]
    assert np.isfinite(surf).all() and (rec[:, 2] >= -1).all()          # every planted null sits in a finished point


# ---- 3. boxes at the end of the plane, fractional coordinates ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cp.PLANE_END_CASES, ids=[cp.case_id(c) for c in cp.PLANE_END_CASES])
def test_search_boxes_that_end_in_the_last_rows_and_columns_of_the_plane(api, case):
    """A check that nothing is disturbed, not a check of values, as tests/test_pixel_phases.py makes it for match_ncc_full: the tile loads
    of all four kernels are clamped to the plane (tlim); the wide kernel's last partial tile reaches furthest past the box.  Two points
    whose box ends in the plane's last row, or in its last column at the last of the four offsets, are appended to the fixture's.  Such a
    box lies wholly in the zero border, so both come back -3, and every other point's record, candidates and surface are byte for byte
    what they are without them."""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    exy, eshift = plane_end_points(f, radius)
    prior = search_shifts(f)[0]
    n = f.xy.shape[0]
    xy, shift = np.ascontiguousarray(np.concatenate([f.xy, exy])), np.ascontiguousarray(np.concatenate([prior, eshift]), np.int32)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for offset in cp.U_OFFSETS:
            offset = np.asarray(offset, np.int32)
            for npeaks in cp.NPEAKS:
                what = f"{cp.case_id(case)}, offset {offset.tolist()}, npeaks {npeaks}"
                want = cp.search(ctx, entry, f.xy, offset, ocw, radius, npeaks, prior, False)
                got = cp.search(ctx, entry, xy, offset, ocw, radius, npeaks, shift, False)
                assert (got[0][n:, 2] == -3).all() and np.isnan(got[2][n:]).all(), what
                assert got[0][:n].tobytes() == want[0].tobytes() and got[2][:n].tobytes() == want[2].tobytes(), what
                if npeaks:
                    assert got[1][:, :n].tobytes() == want[1].tobytes() and (got[1][:, n:, 2] == -3).all(), what
            o_rec, o_surf = cp.oracle_search(f, radius, offset, shift, False, xy=xy)
            cp.vs_oracle(got, o_rec, o_surf, shift, radius, cp.NPEAKS[-1], what + ": vs the oracle")


@pytest.mark.parametrize("case", cp.FRACTIONAL_CASES, ids=[cp.case_id(c) for c in cp.FRACTIONAL_CASES])
def test_searches_truncate(api, case):
    """the reference truncates u and v toward zero: the call on the fractional grid returns the bytes of the call on the truncated grid,
    and the oracle's -- forward and swapped"""
    entry, kind, ocw, radius = case
    f = cp.phase_fixture(case)
    prior = search_shifts(f)[0]
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for swap, seed in ((False, 5), (True, 6)):
            fr = fractional(f.xy, seed)
            sgn = -1 if swap else 1
            o_rec, o_surf = cp.oracle_search(f, radius, sgn * cp.FR_OFFSET, sgn * prior, swap)
            what = f"{cp.case_id(case)}, swap {swap}"
            a = cp.check_call(ctx, entry, f, fr, radius, sgn * cp.FR_OFFSET, sgn * prior, swap, o_rec, o_surf, what + ", fractional grid")
            b = cp.check_call(ctx, entry, f, f.xy, radius, sgn * cp.FR_OFFSET, sgn * prior, swap, o_rec, o_surf, what + ", truncated grid")
            for x, y in zip(a, b):
                assert all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(x, y)), what + ": bytes of the call on the truncated grid"


def test_the_u8_pair_through_the_u16_kernel_is_the_u8_kernels_bytes(api):
    """mode 1 of match_ncc_full_chip_planes takes an 8-bit pair: the phase fixture's u8 pair through both chip kernels, the same bytes"""
    case = ("class", "u8", 11, 7)
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for k in (3, 8):
            offset, shift, swap = calls[k]
            a = cp.search(ctx, "class", f.xy, offset, 11, 7, 4, shift, swap)
            b = cp.search(ctx, "planes", f.xy, offset, 11, 7, 4, shift, swap)
            for x, y, name in zip(a, b, ("record", "candidates", "surface")):
                assert_bits_equal(x, y, f"call {k}: {name}")
            cp.vs_oracle(b, *cp.phase_oracle(case, k), shift, 7, 4, f"call {k}: the u16 kernel vs the oracle")


def test_the_u8_pair_through_the_wide_u16_kernel_is_the_wide_u8_kernels_bytes(api):
    """mode 1 of match_ncc_wide_planes takes an 8-bit pair: the phase fixture's u8 pair through both wide kernels, the same bytes"""
    case = ("wide", "u8", 10, 16)
    f = cp.phase_fixture(case)
    calls = cp.phase_calls(f)
    with api.Context(0) as ctx:
        ctx.set_images(f.i0, f.i1)
        for k in (3, 8):
            offset, shift, swap = calls[k]
            a = cp.search(ctx, "wide", f.xy, offset, 10, 16, 4, shift, swap)
            b = cp.search(ctx, "wplanes", f.xy, offset, 10, 16, 4, shift, swap)
            for x, y, name in zip(a, b, ("record", "candidates", "surface")):
                assert_bits_equal(x, y, f"call {k}: {name}")
            cp.vs_oracle(b, *cp.phase_oracle(case, k), shift, 16, 4, f"call {k}: the wide u16 kernel vs the oracle")
