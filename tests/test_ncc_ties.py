"""Exact ties between f32 NCC values, built in the test: periodic images give bit-equal cells.

DLC: the reference's scan takes the first maximum in u-outer, v-inner order (strict >, :736-741) and the first pivot attaining the
maximum wins (:744-752); the matrix-core kernel replays this with move codes and a DPP arg-max with an index tie-break.
  stripes   images that depend on x alone: every scan is a three-way tie in v, the climbs move (du, -1) until the boundary test stops
            them -- long climbs, past the matrix-core kernel's 16 recorded scans
  tiles     2-D periodic images: period 2 puts ties inside one scan; other periods send pivots to different, equal maxima
Exhaustive search: the first maximum in k = x (2R + 1) + y order, then the border rule (-4).  Period 2 x 2 at R = 15 puts equal maxima at
k = 32 and 34 (one DPP row), 30 (another row) and 96 (the same lane); a phase that puts the first maximum on the border gives -4 although
later ones are interior.  Checked against the oracles and, for the search, against the property itself on a numpy surface."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from full_search_common import assert_records_match, full_search
from ncc_edge_common import fit, surface

MODES = ("auto", "u8px", "u16", "f32", "general")
OCWS = (7, 16, 40)


def periodic(H, W, px, py, seed):
    """i1: a random px x py tile repeated (values 1..255); i0: i1 plus noise (not periodic: the ties come from i1 alone)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tile = rng.integers(1, 256, size=(py, px))
    i1 = np.tile(tile, (H // py + 1, W // px + 1))[:H, :W]
    i0 = np.clip(i1 + rng.integers(-20, 21, size=(H, W)), 1, 255)
    return i0.astype(np.float32), i1.astype(np.float32)


def stripes(H, W, seed):
    """images of x alone: a smooth random profile, i1 the profile moved by 2 px plus noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = np.convolve(rng.standard_normal(W + 40), np.ones(5) / 5, mode="same")[20:W + 20]
    f = np.clip(np.rint(128 + 40 * f / f.std()), 1, 255)
    g = np.clip(np.roll(f, 2) + rng.integers(-3, 4, size=W), 1, 255)
    return np.tile(f, (H, 1)).astype(np.float32), np.tile(g, (H, 1)).astype(np.float32)


def grid(ocw, reach, nx, ny):
    sp = 2 * (ocw + reach) + 3
    m = ocw + reach + 4
    xy = np.zeros((nx * ny, 6))
    for g in range(nx * ny):
        xy[g, :4] = (g % nx, g // nx, m + (g % nx) * sp, m + (g // nx) * sp)
    return xy, 2 * m + (ny - 1) * sp + 1, 2 * m + (nx - 1) * sp + 1


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in lists])
    return off, np.ascontiguousarray(np.concatenate([np.array(p, np.int32).reshape(-1, 2) for p in lists]), np.int32)


# pivot lists (the last one has the largest extent: it sizes the window)
PIVOT_SETS = [
    [(k, 0) for k in range(8)],                               # along u: neighbouring pivots reach neighbouring maxima
    [(0, k) for k in range(-3, 6)],                           # along v
    [(k, k // 2) for k in range(-4, 12)],                     # 16 pivots: one DPP row
    [(k % 5 - 2, k // 5 - 2) for k in range(25)] + [(3, 3)],  # 26 pivots: across rows
    [(1, 0), (0, 12)],                                        # a long window: a long climb
]


def dlc_case(kind, ocw, seed):
    lists = PIVOT_SETS * 2
    reach = 15
    xy, H, W = grid(ocw, reach, 5, 2)
    if kind == "stripes":
        i0, i1 = stripes(H, W, seed)
    else:
        px, py = {"p2": (2, 2), "p3x2": (3, 2), "p5x4": (5, 4)}[kind]
        i0, i1 = periodic(H, W, px, py, seed)
    off, uv = csr(lists)
    return i0, i1, xy, np.array([1, -1], np.int32), off, uv


DLC_KINDS = ("stripes", "p2", "p3x2", "p5x4")


@pytest.mark.parametrize("kind", DLC_KINDS)
@pytest.mark.parametrize("ocw", OCWS)
def test_dlc_ties_oracle_vs_reference(oracle, reference, ocw, kind):
    """CPU: the port oracle equals the compiled reference on the tie cases, both directions."""
    i0, i1, xy, o, off, uv = dlc_case(kind, ocw, 900 + ocw)
    assert_bits_equal(oracle.match(i0, i1, xy, o, off, uv, ocw), reference.match(i0, i1, xy, o, off, uv, ocw), "forward")
    assert_bits_equal(oracle.match(i1, i0, xy, -o, off, -uv, ocw), reference.match(i1, i0, xy, -o, off, -uv, ocw), "swapped")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", DLC_KINDS)
@pytest.mark.parametrize("ocw", OCWS)
def test_dlc_ties_every_path(oracle, ocw, kind, mode):
    from mimc3_amd import api
    i0, i1, xy, o, off, uv = dlc_case(kind, ocw, 900 + ocw)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.set_path(mode)
        got = ctx.matching_ncc_dlc_2(xy, o, off, uv, ocw)
        if mode == "auto":
            assert ctx.last_path() == "u8_mfma"
        assert_bits_equal(got, oracle.match(i0, i1, xy, o, off, uv, ocw), f"{kind} {mode}")
        sw = ctx.matching_ncc_dlc_2(xy, -o, off, -uv, ocw, swap=True)
        assert_bits_equal(sw, oracle.match(i1, i0, xy, -o, off, -uv, ocw), f"{kind} {mode} swapped")


# ---- exhaustive search -------------------------------------------------------------------------------------------------------------------
def full_case(kind, ocw, R, border):
    """(i0, i1, xyuvav, offset): the offset's phase puts the first maximum (in k order) at x = y = 1, or on x = 0 with `border`."""
    xy, H, W = grid(ocw, R, 3, 2)
    if kind == "stripes":
        i0, i1 = stripes(H, W, 3000 + ocw)
        return i0, i1, xy, np.array([-2, 0], np.int32)
    px, py = {"p2": (2, 2), "p3x5": (3, 5), "p7x2": (7, 2)}[kind]
    i0, i1 = periodic(H, W, px, py, 3100 + ocw + R)
    ou = (R - (0 if border else 1)) % px                      # cell x is a maximum where offset + x - R = 0 mod px
    return i0, i1, xy, np.array([ou, (R - 1) % py], np.int32)


def first_max_record(i0, i1, xy, off, ocw, R):
    """The property, from a numpy surface: the lowest k among the cells equal to the maximum -> (k, expected du, dv, peak or -4)"""
    S = 2 * R + 1
    res = []
    for g in range(xy.shape[0]):
        s = surface(i0, i1, xy, off, ocw, g, R).astype(np.float32)
        flat = s.ravel()
        k = int(np.flatnonzero(flat == flat[np.isfinite(flat)].max())[0])
        x, y = divmod(k, S)
        if x in (0, S - 1) or y in (0, S - 1):
            res.append((k, np.nan, np.nan, -4.0))
            continue
        n9 = [s[x - 1 + c, y - 1 + r] for r in range(3) for c in range(3)]
        du, dv = fit(n9, x - R, y - R)
        res.append((k, du, dv, flat[k]))
    return np.array(res)


FULL_CASES = [("p2", 15, False), ("p2", 4, False), ("p3x5", 7, False), ("p7x2", 9, False), ("p3x5", 7, True), ("stripes", 4, False)]


@pytest.mark.parametrize("kind,R,border", FULL_CASES)
@pytest.mark.parametrize("ocw", OCWS)
def test_full_search_ties_oracle(ocw, kind, R, border):
    """CPU: the exhaustive-search oracle picks the lowest tied k (the property on a numpy surface); the cases hold real ties."""
    i0, i1, xy, off = full_case(kind, ocw, R, border)
    out, peak = full_search(i0, i1, xy, off, ocw, R, with_peak=True)
    want = first_max_record(i0, i1, xy, off, ocw, R)
    assert np.array_equal(peak, want[:, 0].astype(np.int32))
    assert_bits_equal(out[:, :3], want[:, 1:].astype(np.float32), f"{kind} R {R}")
    S = 2 * R + 1
    for g in range(xy.shape[0]):
        flat = surface(i0, i1, xy, off, ocw, g, R).astype(np.float32).ravel()
        assert (flat == flat[peak[g]]).sum() >= 2                # a tie
    if border or kind == "stripes":
        assert (out[:, 2] == -4).all()
    else:
        assert (peak == S + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,R,border", FULL_CASES)
@pytest.mark.parametrize("ocw", OCWS)
def test_full_search_ties(ocw, kind, R, border):
    """The matrix-core search against the oracle, both directions, and its forward records against the property itself."""
    from mimc3_amd import api
    i0, i1, xy, off = full_case(kind, ocw, R, border)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        got = ctx.match_ncc_full(xy, off, ocw, R)
        assert ctx.last_path() == "u8_mfma_full"
        sw = ctx.match_ncc_full(xy, -off, ocw, R, swap=True)
    assert_bits_equal(got[:, :3], first_max_record(i0, i1, xy, off, ocw, R)[:, 1:].astype(np.float32), f"{kind} R {R} property")
    assert_records_match(got, full_search(i0, i1, xy, off, ocw, R), f"{kind} R {R}")
    assert_records_match(sw, full_search(i0, i1, xy, -off, ocw, R, swap=True), f"{kind} R {R} swapped")
