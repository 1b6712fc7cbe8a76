"""The point records of the u8 matcher step (U8PointRec, match_kernel.h): u8_classify leaves, at every list position, the header it
has read and derived of that point, and both matcher kernels start from that one record instead of reading the list entry, the point
row, the pivot range, the last pivot and the table queries again.  GPU: path "auto" (records) against the register-tiled kernel alone
("u8px": the memory header) and against the port oracle, bit for bit and in both directions, on pairs of at most 256 x 256 pixels that
aim at what the records carry: list positions around the classifier's 256-thread blocks, a record array of length 0 on either side,
the chip / window roles of the two tables (swap, a non-zero offset), one-wave and four-wave headers, 1 and 64 pivots, corridors wider
than the tile, points the matrix-core kernel appends to the rest list with their record, windows over the image border and void
windows, and the record arrays of two matcher lanes; that the matrix-core kernel really appends points in the cases that aim at it is
read from the kernels' diagnostics.  CPU (test_the_cases_populate_the_lists_they_aim_at, no GPU needed): the inputs of every case are
built and their points classed from the pixels as u8_classify must class them, in both directions, so that the lists a case aims at
are really populated (or really empty)."""
import functools

import numpy as np
import pytest

from conftest import assert_bits_equal
from mimc3_amd import synth
from test_u8_step_lists import stats_run


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def tile_fits(lu, lv, ocw):
    """mx_tile_fit (match_kernel.h) of the DLC tile, origin 1: does the pivot set fit the 32 x 32 cell tile?"""
    ok = True
    for l in (lu, lv):
        d2 = abs(l) + ocw + 2
        cs = 2 * d2 + 1 - 2 * ocw + 1
        c0, c1 = d2 - ocw, d2 - ocw + l
        lo, hi = min(c0, c1), max(c0, c1)
        if cs - 2 > 32:
            # C's integer division truncates; lo + hi is positive here
            t0 = min(max((lo + hi) // 2 - 15, 1), cs - 2 - 31)
            ok = ok and lo - 1 >= t0 and hi + 1 <= t0 + 31
    return ok


def clean_mask(i0, i1, xy, offset, off, uv, ocw, swap=False):
    """True where u8_classify must class the point clean: 1..64 pivots that fit the tile, no null pixel in the chip, none in the
    window's written area (what lies outside the image is the zero border: nulls)"""
    chip, win = (i1, i0) if swap else (i0, i1)
    B = 300
    cz = np.pad(chip == 0, B, constant_values=True)
    wz = np.pad(win == 0, B, constant_values=True)
    out = np.zeros(len(xy), bool)
    for g in range(len(xy)):
        u0, v0 = int(xy[g, 2]), int(xy[g, 3])
        n = int(off[g + 1] - off[g])
        lu, lv = int(uv[off[g + 1] - 1, 0]), int(uv[off[g + 1] - 1, 1])
        dx2, dy2 = abs(lu) + ocw + 2, abs(lv) + ocw + 2
        wu, wv = u0 + int(offset[0]) - dx2 + B, v0 + int(offset[1]) - dy2 + B
        out[g] = (1 <= n <= 64 and tile_fits(lu, lv, ocw) and not cz[v0 - ocw + B:v0 + ocw + 1 + B, u0 - ocw + B:u0 + ocw + 1 + B].any()
                  and not wz[wv:wv + 2 * dy2, wu:wu + 2 * dx2].any())
    return out


def assert_lists(clean, lists, what):
    """the clean and the rest list are populated as the case intends"""
    if lists in ("both", "clean"):
        assert clean.any(), what
    if lists in ("both", "rest"):
        assert (~clean).any(), what
    if lists == "clean":
        assert clean.all(), what
    if lists == "rest":
        assert not clean.any(), what


def check(ctx, oracle, name):
    """auto == u8px == the oracle in both directions; the clean and the rest list are populated as the case intends"""
    i0, i1, xy, offset, off, uv, ocw = build(name)
    got = None
    for swap in (False, True):
        o, p = (-offset, -uv) if swap else (offset, uv)
        clean = clean_mask(i0, i1, xy, o, off, p, ocw, swap)
        print(f"{name} swap {swap}: {int(clean.sum())} clean, {int((~clean).sum())} rest")
        assert_lists(clean, CASES[name], name)
        ctx.set_path("auto")
        res = ctx.matching_ncc_dlc_2(xy, o, off, p, ocw, swap=swap)
        assert ctx.last_path() == "u8_mfma", name
        ctx.set_path("u8px")
        assert_bits_equal(res, ctx.matching_ncc_dlc_2(xy, o, off, p, ocw, swap=swap), f"{name} swap {swap}: auto vs u8px")
        a, b = (i1, i0) if swap else (i0, i1)
        assert_bits_equal(res, oracle.match(a, b, xy, o, off, p, ocw), f"{name} swap {swap}: auto vs oracle")
        got = res if got is None else got
    ctx.set_path("auto")
    return got


def line_pivots(lasts, counts):
    """hand-made pivot lists: point g gets counts[g] pivots on the straight line from (0, 0) to lasts[g]"""
    piv = []
    for (lu, lv), n in zip(lasts, counts):
        t = np.linspace(0.0, 1.0, n) if n > 1 else np.ones(1)
        piv.append(np.stack([np.rint(t * lu), np.rint(t * lv)], axis=1).astype(np.int32))
    off = np.zeros(len(piv) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in piv])
    return off, np.ascontiguousarray(np.concatenate(piv), np.int32)


def stripes(h, w, seed):
    """a stripe pair: NCC surfaces with long ridges, i.e. long climbs"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.arange(w + 40)
    prof = 120.0 + 60.0 * np.sin(x / 3.1) + 30.0 * np.sin(x / 11.0 + 1.0)
    base = np.clip(np.rint(prof[None, :] + rng.integers(-6, 7, (h + 40, w + 40))), 1, 255).astype(np.float32)
    return np.ascontiguousarray(base[20:20 + h, 20:20 + w]), np.ascontiguousarray(base[17:17 + h, 26:26 + w])


# every case and the lists it aims at: "both" populated, only "clean" / only "rest" points, "any"
BLOCK_NS = (1, 255, 256, 257, 513)
CASES = {f"{n}_points": "both" if n > 1 else "any" for n in BLOCK_NS}
CASES.update(only_clean="clean", only_rest="rest", ocw_16="both", ocw_40="both", long_climbs="clean", off_corridor="both",
             fast_among_slow="both", border="both", lanes="both")


@functools.lru_cache(maxsize=None)
def blocks_base():
    """513 points on a 256 x 256 pair with zeroed blobs, ocw 16: prefixes of it are the cases around the classifier's blocks"""
    from mimc3_amd import api
    c = synth.make_small(seed=9100, ocw=16, h=256, w=256, dimx=27, dimy=19, shift=(3, -2), angle_deg=40.0, speed=1700.0, noise_dn=2,
                         null_frac=0.04, offset=(1, -2))
    off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, 16, 256, 256)
    assert c.xyuvav.shape[0] == 513
    return c, off, uv


@functools.lru_cache(maxsize=None)
def lanes_synth():
    """40,000 points on a 256 x 256 pair, ocw 7: more than one chunk of matching_ncc_dlc_cor"""
    c = synth.make_small(seed=9600, ocw=7, h=256, w=256, dimx=200, dimy=200, shift=(3, -2), angle_deg=25.0, speed=1500.0, noise_dn=2,
                         null_frac=0.02, margin=28)
    assert c.xyuvav.shape[0] == 40000
    return c


@functools.lru_cache(maxsize=None)
def build(name):
    """the inputs of a case, built once and left unchanged: (i0, i1, xy, offset, off, uv, ocw)"""
    from mimc3_amd import api
    ocw = 16
    if name.endswith("_points"):
        n = int(name.split("_")[0])
        c, off, uv = blocks_base()
        i0, i1, xy, offset, off, uv = c.i0, c.i1, c.xyuvav[:n], c.offset, off[:n + 1], uv[:off[n]]
    elif name in ("only_clean", "only_rest"):
        # an all-clean pair, and the same pair with a null every 12 pixels: every chip (33 pixels wide) holds one
        c = synth.make_small(seed=9200, ocw=ocw, h=256, w=256, dimx=20, dimy=14, shift=(2, 3), angle_deg=-30.0, speed=1500.0, noise_dn=2,
                             offset=(-1, 2), margin=60)
        if name == "only_rest":
            c.i0[::12, ::12] = 0.0
            c.i1[::12, ::12] = 0.0
        off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, 256, 256)
        i0, i1, xy, offset = c.i0, c.i1, c.xyuvav, c.offset
    elif name in ("ocw_16", "ocw_40"):
        # by turns: 1 pivot, 64 pivots inside the tile, 64 pivots on a corridor wider than the tile, a dozen pivots
        ocw = int(name[4:])
        c = synth.make_small(seed=9300 + ocw, ocw=ocw, h=256, w=256, dimx=8, dimy=8, shift=(3, -2), noise_dn=2, null_frac=0.01,
                             offset=(2, -3), margin=66)
        kinds = [((0, 0), 1), ((13, -9), 64), ((63, -30), 64), ((-11, 6), 12)]
        lasts, counts = zip(*[kinds[(g + g // 8) % 4] for g in range(c.xyuvav.shape[0])])
        off, uv = line_pivots(lasts, counts)
        i0, i1, xy, offset = c.i0, c.i1, c.xyuvav, c.offset
    elif name == "long_climbs":
        i0, i1 = stripes(256, 256, 9400)
        g = np.arange(36)
        xy = np.zeros((36, 6))
        xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3] = g % 6, g // 6, 40 + (g % 6) * 35, 40 + (g // 6) * 35
        lists = [[(1, 0), (0, 12)], [(k, 0) for k in range(8)], [(k, k // 2) for k in range(-4, 12)]]
        piv = [np.array(lists[k % 3], np.int32) for k in range(36)]
        off = np.zeros(37, np.int64)
        off[1:] = np.cumsum([len(p) for p in piv])
        uv = np.ascontiguousarray(np.concatenate(piv), np.int32)
        offset = np.array([1, -1], np.int32)
    elif name in ("off_corridor", "fast_among_slow"):
        # (off_corridor: with this shift the matrix-core launch appends 4 of its 33 listed points in the forward direction)
        c = synth.make_small(seed=9450, ocw=ocw, h=256, w=256, dimx=6, dimy=6, shift=(6, 12) if name == "off_corridor" else (9, 7),
                             angle_deg=45.0, noise_dn=2, null_frac=0.01, speed=2900.0 if name == "off_corridor" else 1600.0, margin=96)
        xy = c.xyuvav.copy()
        if name == "fast_among_slow":
            xy[::5, 4:6] *= 4.5
        off, uv = api.get_uv_pivot(xy, c.dt, c.mpp, ocw, 256, 256)
        last = np.abs(uv[off[1:] - 1]).max(axis=1)
        if name == "off_corridor":
            assert 15 <= int(last.max()) <= 29
        else:
            assert last.max() > 29 and np.median(last) <= 20
        i0, i1, offset = c.i0, c.i1, c.offset
    elif name == "border":
        # chips next to the image edge, windows that hang over it, a void band that makes windows more than 80 % null
        c = synth.make_small(seed=9500, ocw=ocw, h=200, w=210, dimx=8, dimy=7, shift=(2, -2), angle_deg=30.0, speed=1500.0, noise_dn=1,
                             offset=(-2, 1), margin=17)
        c.i1[:, :40] = 0.0
        off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, 200, 210)
        i0, i1, xy, offset = c.i0, c.i1, c.xyuvav, c.offset
    elif name == "lanes":
        ocw = 7
        c = lanes_synth()
        off, uv = api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, 256, 256)
        i0, i1, xy, offset = c.i0, c.i1, c.xyuvav, c.offset
    else:
        raise KeyError(name)
    assert max(i0.shape) <= 256 and i0.shape == i1.shape
    return i0, i1, np.ascontiguousarray(xy), np.asarray(offset, np.int32), off, uv, ocw


@pytest.mark.parametrize("name", list(CASES))
def test_the_cases_populate_the_lists_they_aim_at(name):
    """no GPU: the points of every case, classed from the pixels in the direction(s) the case runs in, fill the lists it aims at"""
    i0, i1, xy, offset, off, uv, ocw = build(name)
    for swap in (False,) if name == "lanes" else (False, True):
        o, p = (-offset, -uv) if swap else (offset, uv)
        clean = clean_mask(i0, i1, xy, o, off, p, ocw, swap)
        print(f"{name} swap {swap}: {int(clean.sum())} clean, {int((~clean).sum())} rest")
        assert_lists(clean, CASES[name], name)
        if name == "lanes":
            assert clean.sum() > 1000 and (~clean).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("n", BLOCK_NS)
def test_list_positions_around_the_classifier_blocks(api, oracle, n):
    """the fill's prefix over blocks puts index and record at the same list position: one point, a block less one, a whole block, a
    block and one, two blocks and one"""
    with api.Context(0) as ctx:
        ctx.set_images(*build(f"{n}_points")[:2])
        check(ctx, oracle, f"{n}_points")


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["clean", "rest"])
def test_a_record_array_of_length_zero(api, oracle, side):
    """an all-clean pair (no rest records) and a pair whose every chip holds a null (no clean records)"""
    with api.Context(0) as ctx:
        ctx.set_images(*build(f"only_{side}")[:2])
        check(ctx, oracle, f"only_{side}")


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", [16, 40])
def test_headers_and_corridors(api, oracle, ocw):
    """the one-wave (ocw 16) and the four-wave (ocw 40) header of the register-tiled kernel, and by turns: 1 pivot, 64 pivots inside the
    tile, 64 pivots on a corridor wider than the tile (straight to the rest list), a dozen pivots; a non-zero offset; blobs of nulls"""
    with api.Context(0) as ctx:
        ctx.set_images(*build(f"ocw_{ocw}")[:2])
        check(ctx, oracle, f"ocw_{ocw}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["long_climbs", "off_corridor", "fast_among_slow"])
def test_points_the_matrix_core_kernel_hands_on(api, oracle, case):
    """points that are on the clean list and leave the matrix-core kernel after it has started -- a climb that outlasts the recorded
    scans (stripes), a climb that leaves a tile that does not cover the cell grid (a shift far off the corridor) -- take their record
    along to the rest list; a few fast points among slow ones sit on the rest list from the start, among the appended ones"""
    with api.Context(0) as ctx:
        ctx.set_images(*build(case)[:2])
        check(ctx, oracle, case)


@pytest.mark.gpu
def test_the_matrix_core_kernel_really_appends():
    """the kernels' diagnostics of one forward call of the off_corridor case (a process of its own: the switch is read once per
    process): the matrix-core launch finishes fewer points than its clean list holds, and exactly the difference is classed kMxRest
    beyond the classifier's rest list afterwards -- so the record copy of an appended point is part of what the case above compares.
    (The stripe case is there for its long climbs; on a 256 x 256 pair at ocw 16 none of them outlasts the recorded scans --
    measured: 36 listed, 36 finished -- so it proves the results of long climbs from records, not the append.)"""
    body = "import test_u8_point_records as r; i0, i1, xy, offset, off, uv, ocw = r.build('off_corridor')"
    c_clean, c_rest, c_nulls, c_wn, l_clean, l_rest, done, rest_after = stats_run(body)
    print("off_corridor: clean list", l_clean, "finished", done, "rest list", l_rest, "kMxRest after the launch", rest_after)
    assert (c_clean, c_rest) == (l_clean, l_rest)
    assert rest_after > l_rest, "no point was appended"
    assert l_clean - done == rest_after - l_rest


@pytest.mark.gpu
def test_windows_over_the_border_and_void_windows(api, oracle):
    """the window origin and the padding arithmetic come from the record: chips next to the image edge, windows that hang over it
    (nulls outside), a void band that makes windows more than 80 % null (status -3), and clean points in the middle"""
    with api.Context(0) as ctx:
        ctx.set_images(*build("border")[:2])
        got = check(ctx, oracle, "border")
    assert (got[:, 2] == -3.0).any() and (got[:, 2] > 0.9).any()


@pytest.mark.gpu
def test_record_arrays_of_two_matcher_lanes(api, oracle):
    """40,000 points through matching_ncc_dlc_cor: three chunks on two matcher lanes, each with lists and records of its own, twice
    (that both lists are more than a thousand long: the CPU test above)"""
    i0, i1, xy, offset, off, uv, ocw = build("lanes")
    c = lanes_synth()
    cor = api.pivot_corridors(xy, c.dt, c.mpp)
    want = oracle.match(i0, i1, xy, offset, off, uv, ocw)
    with api.Context(0) as ctx:
        ctx.set_images(i0, i1)
        ctx.set_path("u8px")
        assert_bits_equal(ctx.matching_ncc_dlc_2(xy, offset, off, uv, ocw), want, "u8px vs oracle")
        ctx.set_path("auto")
        for rep in range(2):
            assert_bits_equal(ctx.matching_ncc_dlc_cor(xy, cor, offset, ocw), want, f"chunked call {rep}")
            assert ctx.last_path() == "u8_mfma"
