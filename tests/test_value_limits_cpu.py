"""CPU: the fixtures of tests/test_value_limits.py earn their place (tests/value_limit_common.py builds them).

a. every pair sits at the top of its class, keeps its nulls, has the class the matcher's path choice predicts, and holds no flat chip;
b. the reference arithmetic alone still finds the displacement on them (the CPU oracles, against the same oracles on the 8-bit pair the
   fixtures were compressed from);
c. the chip-sized box sums reach 99 % of what a chip of `top` pixels sums to, and on 16- and 20-bit pairs the rounding of the f32
   products shows in at least a quarter of the surface cells;
d. the packed summed-area tables of sat_kernel.h, restated in numpy on uint64 with the header's own shifts, return the plain sums of
   every chip-sized box of these pairs -- and stop doing so with any value field one bit narrower;
e. one packed query of the u8 table is exact up to 8,224 pixels and no further: over the 111 x 111 search box of these pairs it
   miscounts the nulls, and the cut into 64 x 64 sub-boxes that sat_nulls_u8_thread makes counts them right."""
import numpy as np
import pytest

from full_dn_common import differing_fraction
from value_limit_common import (CLASSES, DLC_CASES, DLC_NULL_ANGLE, DLC_NULL_OCW, DLC_NULL_SPEED, FIELD_CLASSES, FULL_CASES, FULL_R,
                                PACKED_QUERY_PIXELS, ROUNDING_CLASSES, base_pair, box_sums, case_id, chip_sized_box_maximum, class_pair,
                                dlc_windows, exhaustive_oracle, expected_path, grid_uv, integers, local_ranges, offset_scheme_tried, one_null,
                                pack_f32i_a, pack_u16, pack_u8, rounded_squares, sat_shifts, split_null_count, table, unpack_u16, unpack_u8)

PAIRS = sorted({c[:4] for c in DLC_CASES} | {c[:4] for c in FULL_CASES}, key=str)
CONFIGS = sorted({c[2:4] for c in PAIRS})                  # (ocw, null_frac)
CLASS_PATH = {"u8": "u8_mfma", "u16": "u16_scaled", "f32i": "f32_tiled"}


def prior_shift(c):
    from mimc3_amd import api
    return api.prior_shift(c.xyuvav, c.dt, c.mpp)


# ---- a. fixture properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PAIRS, ids=case_id)
def test_fixture_properties(case):
    kind, spread, ocw, null_frac = case
    top, _, s0, s1, cls, _ = CLASSES[kind]
    c, i0, i1 = class_pair(*case)
    assert i0.dtype == np.float32 and i1.dtype == np.float32
    assert float(i0.max()) == top / s0 and float(i1.max()) == top / s1
    assert np.array_equal(i0 == 0, c.i0 == 0) and np.array_equal(i1 == 0, c.i1 == 0)
    assert ((c.i0 == 0).mean() > 0) == (null_frac > 0)
    q0, q1 = integers(kind, i0, i1)
    for q in (q0, q1):
        assert int(q[q != 0].min()) >= top - spread and int(q.max()) == top
    assert expected_path("auto", i0, ocw, i1) == CLASS_PATH[cls]
    u, v = grid_uv(c.xyuvav)
    assert c.n == 20
    for swap, img in ((False, i0), (True, i1)):               # swapped calls cut their chips from image 1
        for g in range(c.n):
            chip = img[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
            assert chip.shape == (2 * ocw + 1, 2 * ocw + 1)
            assert np.unique(chip[chip != 0]).size >= 2, f"point {g}: a flat chip (swap {swap})"


@pytest.mark.parametrize("ocw", [7, 40])
def test_nine_bit_pairs_fit_the_offset_scheme_or_overflow_it_by_one(oracle, ocw):
    """Spread 254: every chip and window fits a local 8-bit range (1 .. 255 after the offset, 0 being the null).  Spread 255 as a whole:
    no 128 x 128 tile fits, the scheme is not tried.  Spread 255 in one tile: it is tried, some points fit and some overflow by one."""
    c = base_pair(ocw, 0.03)
    H, W = c.i0.shape
    off, uv = oracle.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    for kind, spread, tried in (("9bit", 254, True), ("9bit", 255, False), ("9bit_local", 255, True)):
        _, i0, i1 = class_pair(kind, spread, ocw, 0.03)
        assert offset_scheme_tried(i0, i1) == tried, (kind, spread)
        for a, b, sgn in ((i0, i1, 1), (i1, i0, -1)):
            rc, rw = local_ranges(a, b, c.xyuvav, sgn * c.offset, off, sgn * uv, ocw)
            worst = np.maximum(rc, rw)
            print(f"{kind} spread {spread} ocw {ocw} {'forward' if sgn > 0 else 'swapped'}: {(worst <= 254).sum()} points fit, {(worst == 255).sum()} overflow by one")
            assert worst.max() <= 255
            if spread == 254:
                assert worst.max() <= 254
            if kind == "9bit_local":
                assert (worst <= 254).sum() >= 1 and (worst == 255).sum() >= 1


# ---- b. the reference alone ------------------------------------------------------------------------------------------------------------
def _fits_and_agrees(got, base, what):
    """a fit at every point; at least 90 % of them within 0.5 px of the same oracle on the uncompressed pair"""
    assert (got[:, 2] >= -1).all() and np.isfinite(got[:, :2]).all(), f"{what}: statuses {got[:, 2].tolist()}"
    assert (base[:, 2] >= -1).all(), what + ": the 8-bit pair itself"
    near = float((np.hypot(got[:, 0] - base[:, 0], got[:, 1] - base[:, 1]) <= 0.5).mean())
    print(f"{what}: {near:.2f} of the points within 0.5 px of the 8-bit pair's, peak NCC {got[:, 2].min():.4f} .. {got[:, 2].max():.4f}")
    assert near >= 0.9, what


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"ocw{c[0]}-nulls{c[1]}")
def test_the_reference_alone_finds_the_displacement(oracle, config):
    ocw, null_frac = config
    c = base_pair(ocw, null_frac)
    H, W = c.i0.shape
    off, uv = oracle.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    shift = prior_shift(c)
    base_dlc = {False: oracle.match(c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw),
                True: oracle.match(c.i1, c.i0, c.xyuvav, -c.offset, off, -uv, ocw)}
    base_full = {}
    for kind, spread in sorted({p[:2] for p in PAIRS if p[2:] == config}, key=str):
        _, i0, i1 = class_pair(kind, spread, ocw, null_frac)
        what = f"{kind} spread {spread} ocw {ocw} nulls {null_frac}"
        if (kind, spread, ocw, null_frac) in DLC_CASES:
            _fits_and_agrees(oracle.match(i0, i1, c.xyuvav, c.offset, off, uv, ocw), base_dlc[False], what + ", DLC")
            _fits_and_agrees(oracle.match(i1, i0, c.xyuvav, -c.offset, off, -uv, ocw), base_dlc[True], what + ", DLC swapped")
        for radius in sorted({f[4] for f in FULL_CASES if f[:4] == (kind, spread, ocw, null_frac)}):
            for swap in (False, True):
                sgn = -1 if swap else 1
                # (the 8-bit pair's baseline is the integer oracle for every class: on 8-bit pixels every f32 product is exact and the
                # float-pixel oracle returns the same bytes, which tests/test_full_dn_cpu.py asserts)
                if (radius, swap) not in base_full:
                    base_full[radius, swap] = exhaustive_oracle("u8", c.i0, c.i1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap)[0]
                got = exhaustive_oracle(kind, i0, i1, c.xyuvav, sgn * c.offset, ocw, radius, sgn * shift, swap)[0]
                _fits_and_agrees(got, base_full[radius, swap], what + f", exhaustive R {radius} swap {swap}")


# ---- c. fullness -----------------------------------------------------------------------------------------------------------------------
def tight(kind, spread):
    """the spread leaves the mean pixel within 1 % of the top (the mean sits about spread / 2 below it)"""
    return spread <= 0.016 * CLASSES[kind][0]


FULLNESS = [f for f in FULL_CASES if f[0] in FIELD_CLASSES and tight(f[0], f[1]) and f[4] == FULL_R]


@pytest.mark.parametrize("case", FULLNESS, ids=case_id)
def test_chip_sized_boxes_are_full(case):
    kind, spread, ocw, null_frac, radius = case
    top = CLASSES[kind][0]
    c, i0, i1 = class_pair(kind, spread, ocw, null_frac)
    q0, q1 = integers(kind, i0, i1)
    cw = 2 * ocw + 1
    best = max(chip_sized_box_maximum(q0, q1, c.xyuvav, c.offset, prior_shift(c), ocw, radius),
               chip_sized_box_maximum(q1, q0, c.xyuvav, -c.offset, -prior_shift(c), ocw, radius))
    print(f"{case_id(case)}: largest chip-sized box sum {best} of {cw * cw * top}: {best / (cw * cw * top):.4f}")
    assert best >= 0.99 * cw * cw * top


LOOSE_ROUNDING = [f for f in FULL_CASES if f[0] in ROUNDING_CLASSES and f[1] == CLASSES[f[0]][1][1]]


@pytest.mark.parametrize("case", LOOSE_ROUNDING, ids=case_id)
def test_rounded_products_show_at_the_looser_spread(case):
    """tests/test_full_dn_cpu.py's condition: a kernel that multiplies exactly must not pass"""
    kind, spread, ocw, null_frac, radius = case
    c, i0, i1 = class_pair(kind, spread, ocw, null_frac)
    frac = differing_fraction(i0, i1, c.xyuvav, c.offset, ocw, radius, shift=prior_shift(c))
    print(f"{case_id(case)}: {frac:.3f} of the cells differ between rounded and exact products")
    assert frac >= 0.25


# ---- d. the tables' arithmetic -------------------------------------------------------------------------------------------------------
CW40 = 81


def plain_sums(q):
    """(sum, sum of squares, nulls) of every 81 x 81 box, each in a table of its own: no packing"""
    q = q.astype(np.uint64)
    return (box_sums(table(q), CW40, CW40), box_sums(table(q * q), CW40, CW40), box_sums(table(q == 0), CW40, CW40))


def both_images(kind, spread):
    c, i0, i1 = class_pair(kind, spread, 40, 0.03)
    return integers(kind, i0, i1)


@pytest.mark.parametrize("spread", CLASSES["u8"][1])
def test_u8_table_holds_a_full_chip_and_no_narrower_one_would(spread):
    """word = b | b^2 << 21 | [b == 0] << 50: sum b < 2^21, sum b^2 < 2^29, nulls < 2^13 on a box of 81^2 pixels"""
    sh = sat_shifts()
    sq, nl = sh["kSatSqShift8"], sh["kSatNullShift8"]
    assert CW40 * CW40 * 255 < 2 ** sq and CW40 * CW40 * 255 ** 2 < 2 ** (nl - sq) and CW40 * CW40 < 2 ** 13 <= 2 ** (64 - nl)
    for q in both_images("u8", spread):
        want = plain_sums(q)
        assert (want[2] > 0).any() and (want[2] == 0).any()
        got = unpack_u8(box_sums(table(pack_u8(q, sq, nl)), CW40, CW40), sq, nl)
        for a, b, name in zip(got, want, ("sum", "sum of squares", "nulls")):
            assert np.array_equal(a, b), f"the header's shifts: {name} wrong on {int((a != b).sum())} of {a.size} boxes"
        print(f"u8 spread {spread}: sum b reaches {int(want[0].max()) / 2 ** sq:.4f} of 2^{sq}, sum b^2 {int(want[1].max()) / 2 ** (nl - sq):.4f} of 2^{nl - sq}")
        # the sum field one bit narrower: the square field, and the null field with it, one bit lower
        narrow = unpack_u8(box_sums(table(pack_u8(q, sq - 1, nl - 1)), CW40, CW40), sq - 1, nl - 1)
        assert not all(np.array_equal(a, b) for a, b in zip(narrow, want)), "a 20-bit sum field would do"
        # the square field one bit narrower: the null field one bit lower
        narrow = unpack_u8(box_sums(table(pack_u8(q, sq, nl - 1)), CW40, CW40), sq, nl - 1)
        assert not all(np.array_equal(a, b) for a, b in zip(narrow, want)), "a 28-bit square field would do"


@pytest.mark.parametrize("kind,spread", [(k, s) for k in ("9bit", "12bit", "eighths", "mixed") for s in CLASSES[k][1]])
def test_u16_table_holds_a_full_chip_and_no_narrower_one_would(kind, spread):
    """word = q | q^2 << 25 (q < 4096): sum q < 2^25, sum q^2 < 2^37; the nulls have a table of their own"""
    sq = sat_shifts()["kSatSqShift16"]
    assert CW40 * CW40 * 4095 < 2 ** sq and CW40 * CW40 * 4095 ** 2 < 2 ** 37 and sq + 37 <= 64
    for q in both_images(kind, spread):
        want = plain_sums(q)
        got = unpack_u16(box_sums(table(pack_u16(q, sq)), CW40, CW40), sq, 37)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if kind == "9bit":
            continue                                    # 9-bit values fill no field of this table: theirs is the 8-bit offset scheme
        print(f"{kind} spread {spread}: sum q reaches {int(want[0].max()) / 2 ** sq:.4f} of 2^{sq}, sum q^2 {int(want[1].max()) / 2 ** 37:.4f} of 2^37")
        narrow = unpack_u16(box_sums(table(pack_u16(q, sq - 1)), CW40, CW40), sq - 1, 37)
        assert not (np.array_equal(narrow[0], want[0]) and np.array_equal(narrow[1], want[1])), "a 24-bit sum field would do"
        narrow = unpack_u16(box_sums(table(pack_u16(q, sq)), CW40, CW40), sq, 36)
        assert not np.array_equal(narrow[1], want[1]), "a 36-bit square field would do"


@pytest.mark.parametrize("kind,spread", [(k, s) for k in ROUNDING_CLASSES for s in CLASSES[k][1]])
def test_f32i_table_holds_a_full_chip(kind, spread):
    """a = sum b | nulls << 40, b = sum fl(b * b): sum b < 2^33, nulls < 2^13, sum fl(b * b) < 2^53 on a box of 81^2 pixels.  The sum
    field is wider (40 bits) than its bound (33): what binds on 20-bit pairs is the bound itself, and 2^53, up to which the reference's
    own f64 sums are exact in any order."""
    nl = sat_shifts()["kSatNullShiftF"]
    assert CW40 * CW40 * (2 ** 20 - 1) < 2 ** 33 <= 2 ** nl and CW40 * CW40 < 2 ** 13 <= 2 ** (64 - nl)
    assert CW40 * CW40 * (2 ** 20 - 1) ** 2 < 2 ** 53
    one = np.uint64(1)
    for q in both_images(kind, spread):
        want = plain_sums(q)
        word = box_sums(table(pack_f32i_a(q, nl)), CW40, CW40)
        assert np.array_equal(word & ((one << np.uint64(nl)) - one), want[0]) and np.array_equal(word >> np.uint64(nl), want[2])
        sq = box_sums(table(rounded_squares(q)), CW40, CW40)
        assert int(sq.max()) < 2 ** 53
        if kind == "16bit":
            continue
        print(f"{kind} spread {spread}: sum b reaches {int(want[0].max()) / 2 ** 33:.4f} of 2^33, sum fl(b b) {int(sq.max()) / 2 ** 53:.4f} of 2^53")
        # the top of the class reaches the last bit of both bounds: a 32-bit sum field, or sums exact only below 2^52, would not do
        narrow = box_sums(table(pack_f32i_a(q, 32)), CW40, CW40)
        assert not np.array_equal(narrow >> np.uint64(32), want[2]), "a 32-bit sum field would do"
        assert int(want[0].max()) >= 2 ** 32 and int(sq.max()) >= 2 ** 52
        # and the f64 sum of the rounded squares is that integer, in pixel order as in any other
        y, x = np.unravel_index(int(np.argmax(sq)), sq.shape)
        box = q[y:y + CW40, x:x + CW40].astype(np.float32)
        acc = 0.0
        for p in (box * box).ravel().tolist():
            acc += p
        assert acc == float(int(sq[y, x])) and int(acc) == int(sq[y, x])


# ---- e. the 8,224-pixel rule -----------------------------------------------------------------------------------------------------------
def test_one_packed_query_is_exact_up_to_8224_pixels():
    sh = sat_shifts()
    sq, nl = sh["kSatSqShift8"], sh["kSatNullShift8"]
    n = PACKED_QUERY_PIXELS
    assert n * 255 < 2 ** sq <= (n + 1) * 255 and n * 255 ** 2 < 2 ** (nl - sq)


@pytest.mark.parametrize("spread", CLASSES["u8"][1])
def test_the_whole_search_box_needs_the_split(spread):
    """ocw 40, R 15: the 111 x 111 search box whose null count match_ncc_dlc_mx<Full...> asks for.  At the top of the class its sum of
    pixels passes 2^21 and its sum of squares 2^29, which carries into the null field."""
    sh = sat_shifts()
    sq, nl = sh["kSatSqShift8"], sh["kSatNullShift8"]
    D = 2 * (40 + FULL_R) + 1
    assert D * D > PACKED_QUERY_PIXELS
    for q in both_images("u8", spread):
        S = table(pack_u8(q, sq, nl))
        want = box_sums(table(q == 0), D, D)
        single = box_sums(S, D, D) >> np.uint64(nl)
        wrong = int((single != want).sum())
        print(f"u8 spread {spread}: one packed query over {D} x {D} miscounts the nulls at {wrong} of {want.size} positions")
        assert wrong > 0
        assert np.array_equal(split_null_count(S, nl, D, D), want)
        # what the error is: a carry on top of the count.  A box of at most 111 x 111 pixels that overflows holds at most 4,096 nulls, so
        # the count never wraps to 0: a null-free box reads as holding nulls (the point leaves the clean form), never the reverse
        carry = single.astype(np.int64) - want.astype(np.int64)
        print(f"u8 spread {spread}: the single query's error is {sorted(set(carry.ravel().tolist()))}")
        assert carry.min() >= 0 and carry.max() <= 2 and ((want == 0) & (single > 0)).any()
    # the boxes on either side of the limit that the GPU tests use: below it one query is right, and split_null_count makes one query
    for w, h in ((89, 89), (90, 90), (91, 91), (92, 92), (92, 90)):
        for q in both_images("u8", spread):
            S = table(pack_u8(q, sq, nl))
            want = box_sums(table(q == 0), w, h)
            assert np.array_equal(split_null_count(S, nl, w, h), want), (w, h)
            if w * h <= PACKED_QUERY_PIXELS:
                assert np.array_equal(box_sums(S, w, h) >> np.uint64(nl), want), (w, h)


def test_mid_range_pairs_cannot_tell():
    """On the uncompressed pair the single query over 111 x 111 is right everywhere: no fixture of synth.texture exercises the split."""
    sh = sat_shifts()
    sq, nl = sh["kSatSqShift8"], sh["kSatNullShift8"]
    c = base_pair(40, 0.03)
    D = 2 * (40 + FULL_R) + 1
    for img in (c.i0, c.i1):
        q = img.astype(np.uint64)
        assert np.array_equal(box_sums(table(pack_u8(q, sq, nl)), D, D) >> np.uint64(nl), box_sums(table(q == 0), D, D))


# ---- one null in an otherwise null-free pair: the points that see it get another record --------------------------------------------------
def planted_nulls(c, ocw):
    """(x, y) in image 1 of a null outside every chip-sized centre of a search box but inside point 6's box, and (x, y) in image 0 of a
    null inside point 13's chip"""
    u, v = grid_uv(c.xyuvav)
    return (int(u[6]) + ocw + 9, int(v[6]) - ocw - 6), (int(u[13]) + 3, int(v[13]) - 4)


@pytest.mark.parametrize("ocw", [30, 40])
def test_one_null_changes_the_exhaustive_record(ocw):
    c, i0, i1 = class_pair("u8", 1, ocw, 0.0)
    assert (i0 != 0).all() and (i1 != 0).all()
    shift = prior_shift(c)
    u, v = grid_uv(c.xyuvav)
    clean = exhaustive_oracle("u8", i0, i1, c.xyuvav, c.offset, ocw, FULL_R, shift)[0]
    (bx, by), (cx, cy) = planted_nulls(c, ocw)
    h = ocw + FULL_R
    in_box = (np.abs(u + c.offset[0] + shift[:, 0] - bx) <= h) & (np.abs(v + c.offset[1] + shift[:, 1] - by) <= h)
    in_chip_area = (np.abs(u + c.offset[0] + shift[:, 0] - bx) <= ocw) & (np.abs(v + c.offset[1] + shift[:, 1] - by) <= ocw)
    assert in_box[6] and not in_chip_area[6]
    a = exhaustive_oracle("u8", i0, one_null(i1, bx, by), c.xyuvav, c.offset, ocw, FULL_R, shift)[0]
    changed = (a.view(np.uint32) != clean.view(np.uint32)).any(axis=1)
    assert np.array_equal(changed, in_box), (changed.tolist(), in_box.tolist())
    in_chip = (np.abs(u - cx) <= ocw) & (np.abs(v - cy) <= ocw)
    assert in_chip[13]
    b = exhaustive_oracle("u8", one_null(i0, cx, cy), i1, c.xyuvav, c.offset, ocw, FULL_R, shift)[0]
    changed = (b.view(np.uint32) != clean.view(np.uint32)).any(axis=1)
    assert np.array_equal(changed, in_chip), (changed.tolist(), in_chip.tolist())


def dlc_null_case(oracle):
    """-> (case, i0, i1, pivots, windows' pixel counts): the u8 pair without nulls at DLC_NULL_OCW under a faster, diagonal a-priori"""
    ocw = DLC_NULL_OCW
    c = base_pair(ocw, 0.0, DLC_NULL_SPEED, DLC_NULL_ANGLE)
    _, i0, i1 = class_pair("u8", 1, ocw, 0.0)
    H, W = i0.shape
    off, uv = oracle.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)
    x, y, w, h = dlc_windows(c.xyuvav, c.offset, off, uv, ocw)
    assert x.min() >= 0 and y.min() >= 0 and (x + w).max() <= W and (y + h).max() <= H
    return c, i0, i1, off, uv, w * h


def dlc_null_points(px):
    """one point whose window is a single query and one whose window is split"""
    return int(np.flatnonzero(px <= PACKED_QUERY_PIXELS)[0]), int(np.flatnonzero(px > PACKED_QUERY_PIXELS)[0])


def test_dlc_windows_lie_on_either_side_of_8224_pixels(oracle):
    c, i0, i1, off, uv, px = dlc_null_case(oracle)
    below, above = int((px <= PACKED_QUERY_PIXELS).sum()), int((px > PACKED_QUERY_PIXELS).sum())
    print(f"ocw {DLC_NULL_OCW}, speed {DLC_NULL_SPEED}, angle {DLC_NULL_ANGLE}: {below} windows of at most 8,224 px, {above} beyond; sizes {sorted(set(px.tolist()))}")
    assert below >= 3 and above >= 3
    ocw = DLC_NULL_OCW
    u, v = grid_uv(c.xyuvav)
    clean = oracle.match(i0, i1, c.xyuvav, c.offset, off, uv, ocw)
    for g in dlc_null_points(px):
        # a null next to the window's centre, under every chip-sized box the climb visits; and one in the chip
        wx, wy = int(u[g]) + int(c.offset[0]) + 4, int(v[g]) + int(c.offset[1]) - 5
        a = oracle.match(i0, one_null(i1, wx, wy), c.xyuvav, c.offset, off, uv, ocw)
        assert (a[g].view(np.uint32) != clean[g].view(np.uint32)).any(), f"point {g}: the window's null does not show"
        b = oracle.match(one_null(i0, int(u[g]) + 3, int(v[g]) - 4), i1, c.xyuvav, c.offset, off, uv, ocw)
        assert (b[g].view(np.uint32) != clean[g].view(np.uint32)).any(), f"point {g}: the chip's null does not show"
