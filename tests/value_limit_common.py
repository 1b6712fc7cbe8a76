"""Fixtures at the top of every integer pixel class, shared by tests/test_value_limits_cpu.py and tests/test_value_limits.py.

Every integer kernel is bit-exact because its sums are exact integers that fit the field or the lane they are kept in (the packed
summed-area tables of sat_kernel.h, the 32-bit partial sums of the register-tiled and matrix-core kernels).  The fixtures of
synth.texture sit around mid-range; these compress the same pairs linearly against the top of each class, so that every field carries
what its comment allows: nulls stay 0, every other pixel p of the 8-bit pair becomes (top - rint((255 - p) * spread / 254)) / scale.

Also here: the DLC matcher's expected kernel path per pair and path mode (moved from tests/test_match_parity.py, which imports it), the
tables of sat_kernel.h restated in numpy on uint64, and the geometry of chips, search boxes and DLC windows."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U8_OCW = (7, 15, 16, 30, 32, 40)       # chip sizes the exact u8 kernel is instantiated for
F32T_OCW = (7, 15, 16, 30, 32, 40)     # chip sizes of the register-tiled f32 kernel


def expected_path(mode, i0, ocw, i1=None):
    imgs = [i0] if i1 is None else [i0, i1]
    is_u8 = all(float(i.max()) <= 255.0 and float(i.min()) >= 0 and np.array_equal(i, np.rint(i)) for i in imgs)
    is_si = all(float(i.min()) >= 0 and ((float(i.max()) <= 4095.0 and np.array_equal(i, np.rint(i))) or
                (float(i.max()) * 8 <= 4095.0 and np.array_equal(i * 8, np.rint(i * 8)))) for i in imgs)
    if mode in ("auto", "u8px") and ocw in U8_OCW and is_u8:
        return "u8_mfma" if mode == "auto" else "u8_exact"     # the matrix-core kernel first ("auto"), or the register-tiled kernel alone
    if ocw in U8_OCW and ((mode in ("auto", "u8px") and is_si and not is_u8) or (mode == "u16" and is_u8)):
        return "u16_scaled"
    return "f32_tiled" if (mode != "general" and ocw in F32T_OCW) else "general_f32"


def offset_scheme_tried(i0, i1):
    """capi.cpp's rule for trying the u8 kernels through per-point offsets on a scaled-integer pair ("u8_offset" instead of
    "u16_scaled"): both images integral (shift 0), and in each at least half of the 128 x 128 tiles that hold a non-null pixel have a
    non-null range of at most 254."""
    for img in (i0, i1):
        if not np.array_equal(img, np.rint(img)):
            return False
        fit = total = 0
        for y in range(0, img.shape[0], 128):
            for x in range(0, img.shape[1], 128):
                t = img[y:y + 128, x:x + 128]
                t = t[t != 0]
                if t.size:
                    total += 1
                    fit += int(t.max() - t.min() <= 254)
        if 2 * fit < total:
            return False
    return True


def expected_path_at_limits(mode, i0, i1, ocw):
    """expected_path, and "u8_offset" where the scaled-integer pair is tried through per-point offsets first (modes auto and u8px)."""
    path = expected_path(mode, i0, ocw, i1)
    if path == "u16_scaled" and mode in ("auto", "u8px") and offset_scheme_tried(i0, i1):
        return "u8_offset"
    if mode == "u16" and expected_path("auto", i0, ocw, i1) == "u16_scaled":
        return "u16_scaled"                                  # (the forced u16 kernel takes every scaled-integer pair, not 8-bit ones alone)
    return path


MODES = ("auto", "u8px", "u16", "f32", "general")


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------
def top_of_class(img8, top, spread, scale=1):
    """An 8-bit image (0 = null) against the top of a class: nulls stay 0, every other pixel p becomes
    (top - rint((255 - p) * spread / 254)) / scale as f32 -- p = 255 is `top`, p = 1 is `top - spread`."""
    img8 = np.asarray(img8, np.float64)
    v = (top - np.rint((255.0 - img8) * spread / 254.0)) / scale
    out = np.where(img8 == 0, 0.0, v).astype(np.float32)
    assert np.array_equal(out.astype(np.float64) * scale, np.where(img8 == 0, 0.0, v * scale))       # exact in f32
    return np.ascontiguousarray(out)


NULL_FRACS = (0.0, 0.03, 0.10)
SEEDS = {}          # (ocw, null_frac) -> seed, where 7100 + ocw does not satisfy tests/test_value_limits_cpu.py's conditions


@functools.lru_cache(maxsize=None)
def base_pair(ocw, null_frac, speed=700.0, angle_deg=40.0):
    """full_multi_common.parity_case's pair and grid (20 points, a nearly white texture), the seed free of null_frac and radius"""
    from mimc3_amd import synth
    c = synth.make_small(seed=SEEDS.get((ocw, null_frac), 7100 + ocw), shift=(3, -2), angle_deg=angle_deg, ocw=ocw, speed=speed,
                         h=2 * ocw + 200, w=2 * ocw + 210, dimx=5, dimy=4, noise_dn=2, null_frac=null_frac, offset=(1, -1), sigma=0.3)
    c.i0.setflags(write=False); c.i1.setflags(write=False); c.xyuvav.setflags(write=False)
    return c


# kind -> (top, spreads, scale of image 0, scale of image 1, the pixel class, the exhaustive entry's last_path)
CLASSES = {
    "u8": (255, (1, 3), 1, 1, "u8", "u8_mfma_full"),
    "9bit": (511, (254, 255), 1, 1, "u16", "u16_full"),
    "9bit_local": (511, (255,), 1, 1, "u16", "u16_full"),        # spread 255 inside LOCAL_TILE alone, 254 elsewhere
    "12bit": (4095, (3, 63), 1, 1, "u16", "u16_full"),
    "eighths": (4095, (3, 63), 8, 8, "u16", "u16_full"),
    "mixed": (4095, (3, 63), 1, 8, "u16", "u16_full"),           # image 0 12-bit, image 1 in eighths
    "16bit": (65535, (63, 4095), 1, 1, "f32i", "f32i_full"),
    "20bit": (2 ** 20 - 1, (4095, 65535), 1, 1, "f32i", "f32i_full"),
    "20bit_eighths": (2 ** 20 - 1, (4095, 65535), 8, 8, "f32i", "f32i_full"),
}
LOCAL_TILE = (slice(0, 128), slice(0, 128))
FIELD_CLASSES = ("u8", "12bit", "eighths", "mixed", "16bit", "20bit", "20bit_eighths")        # the classes whose top is a bound of a packed field
ROUNDING_CLASSES = ("16bit", "20bit", "20bit_eighths")                               # f32 products round


@functools.lru_cache(maxsize=None)
def class_pair(kind, spread, ocw, null_frac):
    """-> (case, i0, i1): base_pair(ocw, null_frac) compressed against the top of `kind` (read-only arrays, shared among the tests)"""
    top, spreads, s0, s1 = CLASSES[kind][:4]
    assert spread in spreads
    c = base_pair(ocw, null_frac)
    i0, i1 = top_of_class(c.i0, top, spread, s0), top_of_class(c.i1, top, spread, s1)
    if kind == "9bit_local":
        # The spread-255 pair as a whole has a range of 255 in every 128 x 128 tile, and the matcher then does not try the 8-bit offset
        # scheme at all.  With it in one tile alone the scheme is tried, and the points whose chip or window holds both ends of that
        # tile's range overflow it by one: they must come back through the u16 kernel's list.
        y, x = LOCAL_TILE
        a0, a1 = top_of_class(c.i0, top, 254, s0), top_of_class(c.i1, top, 254, s1)
        a0[y, x], a1[y, x] = i0[y, x], i1[y, x]
        i0, i1 = a0, a1
    i0.setflags(write=False); i1.setflags(write=False)
    return c, i0, i1


def integers(kind, i0, i1):
    """the pair as the integers the kernels keep: pixel times the image's scale, int64"""
    s0, s1 = CLASSES[kind][2:4]
    q0, q1 = i0.astype(np.float64) * s0, i1.astype(np.float64) * s1
    assert np.array_equal(q0, np.rint(q0)) and np.array_equal(q1, np.rint(q1))
    return q0.astype(np.int64), q1.astype(np.int64)


def exhaustive_oracle(kind, i0, i1, xy, offset, ocw, radius, shift, swap=False):
    """The class's CPU oracle of the exhaustive search at npeaks 8 -> (record [N][8], candidates [8][N][3]): the integer oracle on 8-bit
    pairs and, on the pixels times their scale, on 12-bit pairs and eighths (tests/test_full_planes.py does the same); the oracle on
    float pixels, with the reference's rounded f32 products, on 16- and 20-bit pairs."""
    from full_dn_common import full_dn
    from full_multi_common import full_multi
    if CLASSES[kind][4] == "f32i":
        return full_dn(i0, i1, xy, offset, ocw, radius, 8, shift=shift, swap=swap)
    q0, q1 = integers(kind, i0, i1)
    return full_multi(q0.astype(np.float32), q1.astype(np.float32), xy, offset, ocw, radius, 8, shift=shift, swap=swap)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def grid_uv(xy):
    return xy[:, 2].astype(np.int64), xy[:, 3].astype(np.int64)


def box_sums(S, w, h):
    """every w x h box sum of the image behind the table S (modular uint64, as the kernels' inclusion-exclusion) -> [H - h + 1][W - w + 1]"""
    return S[h:, w:] - S[:-h, w:] - S[h:, :-w] + S[:-h, :-w]


def table(words):
    """summed-area table of a uint64 image, with the zero row and column: (H + 1) x (W + 1)"""
    S = np.zeros((words.shape[0] + 1, words.shape[1] + 1), np.uint64)
    S[1:, 1:] = np.cumsum(np.cumsum(words.astype(np.uint64), axis=0, dtype=np.uint64), axis=1, dtype=np.uint64)
    return S


def chip_sized_box_maximum(q0, q1, xy, offset, shift, ocw, radius):
    """The largest sum of a chip-sized box among the grid's chips (image 0) and the chip-sized boxes of their search boxes (image 1,
    centred on point + offset + a-priori shift, clipped to the image) -> int"""
    cw = 2 * ocw + 1
    b0, b1 = box_sums(table(q0), cw, cw), box_sums(table(q1), cw, cw)         # indexed by the box's top-left pixel
    u, v = grid_uv(xy)
    best = 0
    for g in range(xy.shape[0]):
        best = max(best, int(b0[v[g] - ocw, u[g] - ocw]))
        cu, cv = u[g] + offset[0] + shift[g, 0] - ocw, v[g] + offset[1] + shift[g, 1] - ocw
        y0, y1 = max(cv - radius, 0), min(cv + radius, b1.shape[0] - 1)
        x0, x1 = max(cu - radius, 0), min(cu + radius, b1.shape[1] - 1)
        best = max(best, int(b1[y0:y1 + 1, x0:x1 + 1].max()))
    return best


def local_ranges(i0, i1, xy, offset, piv_off, piv_uv, ocw):
    """per point the non-null range (max - min) of its chip in i0 and of its DLC window in i1 -> two int arrays"""
    u, v = grid_uv(xy)
    x, y, w, h = dlc_windows(xy, offset, piv_off, piv_uv, ocw)
    rc, rw = [], []
    for g in range(xy.shape[0]):
        chip = i0[v[g] - ocw:v[g] + ocw + 1, u[g] - ocw:u[g] + ocw + 1]
        win = i1[max(y[g], 0):y[g] + h[g], max(x[g], 0):x[g] + w[g]]
        chip, win = chip[chip != 0], win[win != 0]
        rc.append(int(chip.max() - chip.min()))
        rw.append(int(win.max() - win.min()))
    return np.array(rc), np.array(rw)


def dlc_windows(xy, offset, piv_off, piv_uv, ocw):
    """The DLC matcher's window of every point, as u8_classify_kernel.hip and the matcher kernels' headers size it from the point's last
    pivot: (x, y, w, h) int arrays in image pixels -- w = 2 (|lu| + ocw + 2), h = 2 (|lv| + ocw + 2), top-left at point + offset - half."""
    u, v = grid_uv(xy)
    last = piv_uv[piv_off[1:] - 1]
    dx2, dy2 = np.abs(last[:, 0]) + ocw + 2, np.abs(last[:, 1]) + ocw + 2
    return u + offset[0] - dx2, v + offset[1] - dy2, 2 * dx2, 2 * dy2


PACKED_QUERY_PIXELS = 8224          # sat_kernel.h: one packed query of the u8 table is exact up to here


# ---- sat_kernel.h in numpy ----------------------------------------------------------------------------------------------------------
def sat_shifts():
    """kSatSqShift8, kSatNullShift8, kSatSqShift16, kSatNullShiftF as sat_kernel.h defines them"""
    src = open(os.path.join(ROOT, "mimc3_amd", "csrc", "sat_kernel.h")).read()
    out = {}
    for name in ("kSatSqShift8", "kSatNullShift8", "kSatSqShift16", "kSatNullShiftF"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m, f"{name} not found in sat_kernel.h"
        out[name] = int(m.group(1))
    return out


def pack_u8(q, sq_shift, null_shift):
    q = q.astype(np.uint64)
    return q + ((q * q) << np.uint64(sq_shift)) + ((q == 0).astype(np.uint64) << np.uint64(null_shift))


def unpack_u8(word, sq_shift, null_shift):
    """-> (sum, sum of squares, nulls) as the kernels cut them out of a box's word"""
    one = np.uint64(1)
    return (word & ((one << np.uint64(sq_shift)) - one), (word >> np.uint64(sq_shift)) & ((one << np.uint64(null_shift - sq_shift)) - one),
            word >> np.uint64(null_shift))


def pack_u16(q, sq_shift):
    q = q.astype(np.uint64)
    return q + ((q * q) << np.uint64(sq_shift))


def unpack_u16(word, sq_shift, sq_bits=64):
    one = np.uint64(1)
    sq = word >> np.uint64(sq_shift)
    if sq_bits < 64 - sq_shift:
        sq = sq & ((one << np.uint64(sq_bits)) - one)
    return word & ((one << np.uint64(sq_shift)) - one), sq


def pack_f32i_a(q, null_shift):
    q = q.astype(np.uint64)
    return q + ((q == 0).astype(np.uint64) << np.uint64(null_shift))


def rounded_squares(q):
    """fl(q * q): the reference's f32 product of a pixel with itself, as an integer"""
    f = q.astype(np.float32)
    return (f * f).astype(np.float64).astype(np.uint64)


def split_null_count(S, null_shift, w, h):
    """sat_nulls_u8_thread for every w x h box of the image behind the packed u8 table S: one query up to PACKED_QUERY_PIXELS pixels, else
    the box cut into sub-boxes of at most 64 x 64 pixels, one query each, the counts added"""
    ny, nx = S.shape[0] - h, S.shape[1] - w
    if w * h <= PACKED_QUERY_PIXELS:
        return box_sums(S, w, h) >> np.uint64(null_shift)
    cnt = np.zeros((ny, nx), np.uint64)
    for j in range(0, h, 64):
        for i in range(0, w, 64):
            w0, h0 = min(w - i, 64), min(h - j, 64)
            sub = box_sums(S, w0, h0)                          # indexed by the sub-box's top-left pixel
            cnt += sub[j:j + ny, i:i + nx] >> np.uint64(null_shift)
    return cnt


# ---- what the GPU tests run, and tests/test_value_limits_cpu.py qualifies: (kind, spread, ocw, null_frac) ------------------------------
def _dlc_cases():
    cases = []
    for spread in CLASSES["u8"][1]:
        cases += [("u8", spread, ocw, nf) for ocw in U8_OCW for nf in (0.0, 0.03)]
        cases += [("u8", spread, ocw, 0.10) for ocw in (30, 40)]          # the sparse null lists of PxU8, full
    for spread in CLASSES["12bit"][1]:
        cases += [("12bit", spread, ocw, 0.03) for ocw in (7, 16, 30, 40)]
        cases += [("12bit", spread, ocw, 0.10) for ocw in (30, 40)]
    for kind in ("9bit", "9bit_local", "eighths", "16bit", "20bit", "20bit_eighths"):
        cases += [(kind, spread, ocw, 0.03) for spread in CLASSES[kind][1] for ocw in (7, 40)]
    cases += [("mixed", 3, ocw, 0.03) for ocw in (7, 40)]
    cases += [(kind, CLASSES[kind][1][0], 40, 0.0) for kind in CLASSES if kind not in ("u8", "9bit_local")]      # the forms without nulls, on the largest chip
    return cases


FULL_R = 15


def _full_cases():
    """(kind, spread, ocw, null_frac, radius).  The u8 extras straddle PACKED_QUERY_PIXELS with their whole search box:
    ocw 30 at R 14 / 15 and ocw 32 at R 12 / 13 are 89^2 = 7,921 / 91^2 = 8,281 pixels."""
    cases = [(kind, spread, ocw, 0.03, FULL_R) for kind in CLASSES if not kind.startswith("9bit") for spread in CLASSES[kind][1] for ocw in (7, 40)]
    cases += [(kind, CLASSES[kind][1][0], 40, 0.0, FULL_R) for kind in CLASSES if not kind.startswith("9bit")]
    cases += [("u8", 1, 30, 0.03, 14), ("u8", 1, 30, 0.03, 15), ("u8", 1, 32, 0.03, 12), ("u8", 1, 32, 0.03, 13)]
    return cases


DLC_CASES = _dlc_cases()
FULL_CASES = _full_cases()


def case_id(case):
    return "-".join(str(x) for x in case)


# ---- one null in an otherwise null-free pair -------------------------------------------------------------------------------------------
DLC_NULL_OCW, DLC_NULL_SPEED, DLC_NULL_ANGLE = 30, 1650.0, 45.0      # a corridor whose windows are 90 x 90 (one query) and 92 x 92 (split)


def one_null(img, x, y):
    out = np.array(img, np.float32)
    assert out[y, x] != 0
    out[y, x] = 0
    return np.ascontiguousarray(out)
