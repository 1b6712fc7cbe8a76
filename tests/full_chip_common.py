"""Test infrastructure of the exhaustive search at any chip size (mimc3_match_ncc_full_chip, match_full_chip_kernel.hip): the band rule of
the kernel in Python terms, the fixtures the CPU and GPU tests share -- the makers of full_multi_common, full_dn_common and
full_any_common at a chip size of the caller's, with PLACED nulls for chips of 81 px and more, where null blobs leave no clean point --
the per-band classification of a point as the kernel decides it, and the list of every fixture a GPU test uses (tests/test_full_chip_cpu.py
counts their clean, dirty and fitted points without a device)."""
import numpy as np

from full_any_common import encode_nulls, float_case, wide_case
from full_dn_common import dn16_case
from full_multi_common import STATUS_R, parity_case
from null_encoding_common import first_invalid_count

PATH = "f32g_chip"
MAX_OCW = 80
LDS_BUDGET = 79 * 1024                  # kChipLdsBudget (match_kernel.h)
KINDS = ("u8", "u16", "float", "wide")
EXACT = {"u8": True, "u16": True, "float": True, "wide": False}       # exact f64 sums: the oracle's surface bit for bit
PLACED_FROM = 40                        # chips of 81 px and more take placed nulls
# null fraction of the blob fixtures per chip size: chosen so that every fixture the GPU tests use keeps >= 3 clean and >= 3 dirty points
BLOB_FRAC = {1: 0.06, 2: 0.06, 3: 0.06, 7: 0.04, 10: 0.03, 11: 0.03, 16: 0.03, 20: 0.02}


# ---- the band rule (include/mimc3_hip.h, match_full_chip_kernel.hip chip_layout) ----
def layout(ocw, radius):
    """-> dict(CW, CWP, PB, BR, lds): chip width, its pitch, the box row pitch, the band height and the launch's dynamic LDS bytes"""
    cw = 2 * ocw + 1
    cwp = (cw + 3) & ~3
    bw = cwp + 32
    pb = bw if (bw // 4) & 1 else bw + 4
    row, fixed = 4 * (pb + cwp), 4 * 2 * radius * pb
    br = min((LDS_BUDGET - fixed) // row, cw)
    lds = (4 * (br + 2 * radius) * pb + max(4 * br * cwp, 4 * 32 * 33) + 15) & ~15
    return dict(CW=cw, CWP=cwp, PB=pb, BR=br, lds=lds)


def band_rows(ocw, radius):
    if not (1 <= ocw <= MAX_OCW and 1 <= radius <= 15):
        return 0
    return layout(ocw, radius)["BR"]


BAND_SHAPES = ("one_band", "one_band_plus_row", "last_band_one_row", "full_last_band")


def band_shape(cw, br):
    """which of BAND_SHAPES a chip of cw rows walked in bands of br rows is, or None"""
    if cw == br:
        return "one_band"
    if cw == br + 1:
        return "one_band_plus_row"
    if cw > 2 * br and cw % br == 1:
        return "last_band_one_row"
    if cw >= 2 * br and cw % br == 0:
        return "full_last_band"
    return None


def band_shape_cases(rows=band_rows):
    """For each of BAND_SHAPES one (ocw, R), derived from the band rule `rows` (the library's query on the GPU side): the largest R that
    has a chip size of that shape, and at that R the largest such ocw.  (At R 15 the rule -- the largest band that fits the budget --
    yields only the first shape: its remainders there are 5 .. 56 rows.  The boundary code does not depend on R.)"""
    found = {}
    for radius in range(15, 0, -1):
        for ocw in range(MAX_OCW, 0, -1):
            s = band_shape(2 * ocw + 1, rows(ocw, radius))
            if s and s not in found:
                found[s] = (ocw, radius)
    return found


# ---- fixtures ----
def placed_nulls(c, shift, ocw, radius):
    """The null pixels of a placed-null fixture, for the unswapped call on the 5 x 4 grid -> ([(row, col)] of image 0, ... of image 1):
    the top-left point gets one null in its chip's first row (its first band alone is dirty), the top-right point one in the last
    column of its box (box row 1), the bottom-right point one in the last row of its box (its last band alone), the bottom-left point
    one in the first column of its box every 16 rows (every band).  The interior points stay clean."""
    xy, h = c.xyuvav, ocw + radius
    def uv(g):
        return int(xy[g, 2]), int(xy[g, 3])
    def centre(g):
        u, v = uv(g)
        return u + int(c.offset[0]) + int(shift[g, 0]), v + int(c.offset[1]) + int(shift[g, 1])
    tl, tr, bl, br = 0, c.dimx - 1, (c.dimy - 1) * c.dimx, c.dimx * c.dimy - 1
    u, v = uv(tl)
    p0 = [(v - ocw, u - ocw + 1)]
    cu, cv = centre(tr)
    p1 = [(cv - h + 1, cu + h)]
    cu, cv = centre(br)
    p1.append((cv + h, cu + h - 1))
    cu, cv = centre(bl)
    p1 += [(cv - h + y, cu - h) for y in range(0, 2 * h + 1, 16)]
    return p0, p1


def chip_case(kind, ocw, radius, encoding="zero"):
    """One pair and grid (5 x 4 points, image (2 ocw + 200) x (2 ocw + 210)) at any chip size -> (case, i0, i1, a-priori shift).
    kind: "u8" parity_case, "u16" dn16_case (full low-order entropy), "float" float_case, "wide" the six-decade wide_case; nulls are
    blobs (BLOB_FRAC) below PLACED_FROM and placed_nulls from there on; encoding (float kinds): one of full_any_common.ENCODINGS."""
    placed = ocw >= PLACED_FROM
    frac = 0.0 if placed else BLOB_FRAC[ocw]
    if kind == "u8":
        c, shift = parity_case(ocw, frac, radius, dimx=5, dimy=4)
        i0, i1 = c.i0.copy(), c.i1.copy()
    elif kind == "u16":
        c, i0, i1, shift = dn16_case(ocw, frac, radius)
    else:
        c, i0, i1, shift = (float_case if kind == "float" else wide_case)(ocw, frac, radius, "zero")
    if placed:
        p0, p1 = placed_nulls(c, shift, ocw, radius)
        for img, px in ((i0, p0), (i1, p1)):
            for y, x in px:
                img[y, x] = 0
    if kind in ("float", "wide"):
        i0, i1 = encode_nulls(i0, i1, encoding)
    else:
        assert encoding == "zero"
    return c, np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32), shift


def excluded(img):
    """the inclusion rule's complement: not (double)p >= 1e-10 (a NaN is excluded)"""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(img, np.float64) >= 1e-10)


def band_classes(i0, i1, xy, offset, shift, ocw, radius, swap=False, rows=band_rows):
    """Per point the list of its bands' bodies as the kernel chooses them: True = dirty (an excluded pixel among the band's chip rows
    or the box rows they meet), False = clean.  Box pixels outside the image are the planes' zero border, i.e. excluded."""
    a, b = (i1, i0) if swap else (i0, i1)
    ea, eb = excluded(a), excluded(b)
    H, W = a.shape
    h, cw, br = ocw + radius, 2 * ocw + 1, rows(ocw, radius)
    out = []
    for g in range(xy.shape[0]):
        u, v = int(xy[g, 2]), int(xy[g, 3])
        cu = u + int(offset[0]) + (0 if shift is None else int(shift[g, 0]))
        cv = v + int(offset[1]) + (0 if shift is None else int(shift[g, 1]))
        chip = ea[v - ocw:v + ocw + 1, u - ocw:u + ocw + 1]
        box = np.ones((2 * h + 1, 2 * h + 1), bool)
        y0, y1, x0, x1 = max(cv - h, 0), min(cv + h + 1, H), max(cu - h, 0), min(cu + h + 1, W)
        if y1 > y0 and x1 > x0:
            box[y0 - (cv - h):y1 - (cv - h), x0 - (cu - h):x1 - (cu - h)] = eb[y0:y1, x0:x1]
        out.append([bool(chip[r0:r0 + br].any() or box[r0:min(r0 + br, cw) + 2 * radius].any()) for r0 in range(0, cw, br)])
    return out


def class_counts(bands):
    """-> (points with every band clean, points with a dirty band, of those the points that also have a clean band)"""
    clean = sum(1 for b in bands if not any(b))
    dirty = sum(1 for b in bands if any(b))
    mixed = sum(1 for b in bands if any(b) and not all(b))
    return clean, dirty, mixed


def only_null_in_last_box_line(i1, xy, offset, shift, ocw, radius):
    """-> (points whose box's only excluded pixel lies in its last row, ... in its last column); the unswapped call, boxes inside the image"""
    e, h = excluded(i1), ocw + radius
    last_row, last_col = [], []
    for g in range(xy.shape[0]):
        cu = int(xy[g, 2]) + int(offset[0]) + int(shift[g, 0])
        cv = int(xy[g, 3]) + int(offset[1]) + int(shift[g, 1])
        box = e[cv - h:cv + h + 1, cu - h:cu + h + 1]
        if box.sum() == 1:
            if box[-1].any():
                last_row.append(g)
            if box[:, -1].any():
                last_col.append(g)
    return last_row, last_col


# ---- statuses at a chip size of the caller's ----
def chip_status_case(ocw):
    """full_multi_common.status_case's geometry at chip half-width ocw, for R = STATUS_R and offset (0, 0): image 1 is image 0 moved by
    (+5, 0), so an ordinary point's true offset is a border cell of the search.  Point 0's box has exactly the first null count beyond
    80 % (-3), point 1's chip is flat (-2: no finite cell), point 2 is ordinary (-4, with the interior local maxima of a rough surface),
    points 3-5 overhang the left, bottom-right and top image edges, point 6 has the a-priori shift (3, 1) and so an interior peak (a fit).
    -> (i0, i1, xyuvav, shift int32[7][2])"""
    from mimc3_amd import synth
    R = STATUS_R
    h, cw = ocw + R, 2 * ocw + 1
    D = 2 * h + 1
    cell = D + 12
    H = W = 3 * cell
    i0 = synth.texture(H, W, 300 + ocw, sigma=0.5)
    i1 = np.roll(i0, (0, 5), axis=(0, 1)).copy()
    c = [cell // 2 + k * cell for k in range(3)]
    xy = np.zeros((7, 6))
    xy[:, 2:4] = [[c[0], c[0]], [c[1], c[0]], [c[2], c[0]], [ocw, c[1]], [W - 1 - ocw, H - 1 - ocw], [c[2], ocw], [c[1], c[1]]]
    k = first_invalid_count(D * D)
    box = i1[c[0] - h:c[0] + h + 1, c[0] - h:c[0] + h + 1]
    idx = np.random.default_rng(ocw).choice(D * D, k, replace=False)
    box[np.unravel_index(idx, box.shape)] = 0
    i0[c[0] - ocw:c[0] + ocw + 1, c[1] - ocw:c[1] + ocw + 1] = 9
    shift = np.zeros((7, 2), np.int32)
    shift[6] = (3, 1)
    return np.ascontiguousarray(i0, np.float32), np.ascontiguousarray(i1, np.float32), xy, shift


# ---- every fixture a GPU test of tests/test_full_chip.py uses: (kind, ocw, R, encoding, swap) ----
SMALL_OCW = (1, 2, 3, 10, 11)           # CW below two chunks; both values of CWP - CW
RADII = (1, 4, 7, 15)
MODE1_OCW = (7, 16, 40)
ENC = ("zero", "nan_zero", "m9999_nan")


def small_fixtures():
    """the small chips: every kind at R 15 and R 4, both ways round; the float kinds in the three encodings"""
    out = []
    for i, ocw in enumerate(SMALL_OCW):
        for kind in KINDS:
            enc = ENC[i % 3] if kind in ("float", "wide") else "zero"
            out += [(kind, ocw, 15, enc, False), (kind, ocw, 4, enc, True)]
    return out


def radius_fixtures():
    """every radius at ocw 10 and 11, on the wide-range pair in the three encodings and on the 16-bit pair"""
    out = []
    for ocw in (10, 11):
        for i, radius in enumerate(RADII):
            out += [("wide", ocw, radius, ENC[(i + ocw) % 3], bool(i & 1)), ("u16", ocw, radius, "zero", not (i & 1))]
    return out


def band_fixtures(rows=band_rows):
    """the band-boundary chip sizes and the LDS ceiling (64 and 80 at R 15 and R 1): 16-bit (exact) and the wide-range pair"""
    sizes = [band_shape_cases(rows)[s] for s in BAND_SHAPES] + [(64, 15), (80, 15), (64, 1), (80, 1)]
    out = []
    for i, (ocw, radius) in enumerate(sizes):
        out += [("u16", ocw, radius, "zero", False), ("wide", ocw, radius, ENC[i % 3], False)]
    out += [("u8", 80, 15, "zero", False), ("float", 64, 15, "nan_zero", False)]
    return out


def mode1_fixtures():
    out = []
    for ocw in MODE1_OCW:
        out += [(kind, ocw, 15 if ocw != 16 else 7, "zero", False) for kind in KINDS]
    return out
