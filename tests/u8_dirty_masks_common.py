"""Test infrastructure: tiny 8-bit pairs whose window nulls sit where the register-tiled kernel's masked bodies can go wrong, and the
numpy restatement of the byte-mask helper those bodies are built on (match_px_kernel.hip: nzff, PxU8::task).

Every fixture is a dozen points of zero velocity on one small pair: the pivots are (0, 0) .. (10, 0), so a point's search area is
Dx2 x Dy2 = (2 (ocw + 12) + 1) x (2 (ocw + 2) + 1) with its top-left pixel at uv0 - (Dx2 / 2, Dy2 / 2), its last row and column are
never written (T4), and cell (cx, cy) -- the chip laid with its origin on window pixel (cx, cy) -- is displacement (cx - 12, cy - 2).
The 3 x 3 scans of the eleven pivot starts evaluate cells cx 11 .. 23, cy 1 .. 3 of every valid point whatever the surface looks like
(the "certain set"); a climb that ends on dv = +1 has scanned the T4 row (cy = 4), one that ends on du = +11 the T4 column (cx = 24).
The points are 7 px apart in u, so their windows start at all four byte phases, and the scans' boxes at every phase again.

Window coordinates below are those of point 0."""
import dataclasses

import numpy as np

from mimc3_amd import synth
import null_encoding_common as nc

KINDS = ("single_phases", "box_sides", "carry", "blob_edge", "t4_row", "t4_col", "both_sides", "one_valid_limit")
SHIFT = {"t4_row": (-2, 1), "t4_col": (11, 0)}          # where the surface peaks (du, dv); (-2, 0) for every other kind
NEIGHBOURS = ((1, 255), (127, 128), (128, 1), (255, 127))


# ---- the helper, restated ---------------------------------------------------------------------------------------------------------
def nzff_plain(v):
    """0xFF in every byte of the uint32 array v that is non-zero: the per-byte definition."""
    v = np.asarray(v, np.uint32)
    out = np.zeros_like(v)
    for k in range(4):
        out |= np.where((v >> np.uint32(8 * k)) & np.uint32(0xFF), np.uint32(0xFF) << np.uint32(8 * k), np.uint32(0))
    return out


def perm(s0, s1, sel):
    """v_perm_b32: byte k of the result is picked from the eight bytes of {s0, s1} (s1 the low dword) by selector byte k: 0..7 that
    byte, 8 / 9 / 10 / 11 bit 15 / 31 / 47 / 63 replicated over the byte, 12 0x00, 13.. 0xFF."""
    q = (np.asarray(s0, np.uint64) << np.uint64(32)) | np.asarray(s1, np.uint64)
    out = np.zeros(q.shape, np.uint32)
    for k in range(4):
        s = (sel >> (8 * k)) & 0xFF
        if s <= 7:
            b = (q >> np.uint64(8 * s)) & np.uint64(0xFF)
        elif s <= 11:
            b = ((q >> np.uint64(15 + 16 * (s - 8))) & np.uint64(1)) * np.uint64(0xFF)
        else:
            b = np.full(q.shape, 0 if s == 12 else 0xFF, np.uint64)
        out |= b.astype(np.uint32) << np.uint32(8 * k)
    return out


def pk_add_u16_sat(a, b):
    """v_pk_add_u16 with clamp: both half-words added, each saturating at 0xffff."""
    a = np.asarray(a, np.uint32); b = np.asarray(b, np.uint32)
    lo = np.minimum((a & np.uint32(0xFFFF)).astype(np.uint64) + (b & np.uint32(0xFFFF)), 0xFFFF)
    hi = np.minimum((a >> np.uint32(16)).astype(np.uint64) + (b >> np.uint32(16)), 0xFFFF)
    return (lo | (hi << np.uint64(16))).astype(np.uint32)


def nzff(v, sel=0x0B090A08, shift_hi=0x7F007F00):
    """The kernel's four instructions, one numpy line each."""
    v = np.asarray(v, np.uint32)
    e = (v & np.uint32(0x00FF00FF)) + np.uint32(0x7FFF7FFF)          # wraps modulo 2^32 like v_add_u32 (it never does)
    o = pk_add_u16_sat(v, np.uint32(shift_hi))
    return perm(o, e, sel)


def dot4(a, b):
    a = np.asarray(a, np.uint32); b = np.asarray(b, np.uint32)
    s = np.zeros(a.shape, np.uint64)
    for k in range(4):
        s += ((a >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.uint64) * ((b >> np.uint32(8 * k)) & np.uint32(0xFF))
    return s


def body_sums(a, bw, chip_mask=None):
    """The six sums of one dword task as the rewritten bodies form them (chip_mask: the pad mask of a GC row task; None = derived
    from the chip dword as GENERAL does).  n comes back in pixels (the kernel counts eight per pixel and shifts once per lane)."""
    a = np.asarray(a, np.uint32); bw = np.asarray(bw, np.uint32)
    mb = nzff(bw)
    mf = nzff(a) if chip_mask is None else np.uint32(chip_mask)
    am, bm = a & mb, bw & mf
    ones = np.uint32(0x01010101)
    pop = np.array([bin(int(x)).count("1") for x in (mb & mf).reshape(-1)], np.uint64).reshape(a.shape)
    return dict(n=pop >> np.uint64(3), sx=dot4(am, ones), sy=dot4(bm, ones), sxx=dot4(am, a), syy=dot4(bm, bw), sxy=dot4(a, bw))


def plain_sums(a, bw, chip_mask=None):
    """The same sums from the definition: a pixel takes part iff its chip byte is valid (non-zero, or inside the pad mask) and its
    window byte is non-zero; sx, sxx run over chip bytes, sy, syy over window bytes, of the pixels that take part."""
    a = np.asarray(a, np.uint32); bw = np.asarray(bw, np.uint32)
    out = {k: np.zeros(a.shape, np.uint64) for k in ("n", "sx", "sy", "sxx", "syy", "sxy")}
    for k in range(4):
        x = ((a >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.uint64)
        y = ((bw >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.uint64)
        cv = (x != 0) if chip_mask is None else np.full(a.shape, bool((chip_mask >> (8 * k)) & 0xFF))
        x = np.where(cv, x, 0)                     # (pad bytes of a chip dword are 0 anyway)
        ok = cv & (y != 0)
        out["n"] += ok
        out["sx"] += np.where(ok, x, 0); out["sxx"] += np.where(ok, x * x, 0)
        out["sy"] += np.where(ok, y, 0); out["syy"] += np.where(ok, y * y, 0)
        out["sxy"] += x * y
    return out


def edge_dwords():
    """Every byte value at each of the four byte positions, with each of the three other bytes in {0, 1, 0x7f, 0x80, 0xff}:
    4 x 256 x 125 dwords (the helper works byte by byte or half-word by half-word, so a fault needs no more than one neighbour)."""
    nb = np.array([0, 1, 0x7F, 0x80, 0xFF], np.uint32)
    vals = np.arange(256, dtype=np.uint32)
    out = []
    for pos in range(4):
        others = [p for p in range(4) if p != pos]
        g = np.meshgrid(vals, nb, nb, nb, indexing="ij")
        d = g[0] << np.uint32(8 * pos)
        for p, x in zip(others, g[1:]):
            d = d | (x << np.uint32(8 * p))
        out.append(d.reshape(-1))
    return np.concatenate(out)


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------
def geometry(ocw):
    return 2 * (ocw + 12) + 1, 2 * (ocw + 2) + 1, 2 * ocw + 1          # Dx2, Dy2, cw


@dataclasses.dataclass
class MaskCase:
    kind: str
    ocw: int
    chip_img: np.ndarray
    win_img: np.ndarray
    xyuvav: np.ndarray
    offset: np.ndarray
    x0: int                   # image coordinates of point 0's window pixel (0, 0)
    y0: int

    def window(self, k, img=None):
        """Point k's search area as the matcher sees it: Dy2 x Dx2, T4 row and column zero."""
        Dx2, Dy2, _ = geometry(self.ocw)
        u, v = self.xyuvav[k, 2:4].astype(int)
        w = np.array((self.win_img if img is None else img)[v - Dy2 // 2:v - Dy2 // 2 + Dy2, u - Dx2 // 2:u - Dx2 // 2 + Dx2], np.float32)
        w[-1, :] = 0; w[:, -1] = 0
        return w

    def chip(self, k, img=None):
        u, v = self.xyuvav[k, 2:4].astype(int)
        return (self.chip_img if img is None else img)[v - self.ocw:v + self.ocw + 1, u - self.ocw:u + self.ocw + 1]


def make_case(ocw, kind, lift=0):
    """`lift` is added to every non-null pixel of both images (200: a 9-bit pair whose local ranges fit a byte, i.e. the per-point
    offset policy on the same null geometry)."""
    Dx2, Dy2, cw = geometry(ocw)
    W, H = Dx2 + 30, Dy2 + 26
    du, dv = SHIFT.get(kind, (-2, 0))
    rng = np.random.default_rng(1000 * ocw + KINDS.index(kind))
    base = synth.texture(H + 32, W + 32, 5100 + ocw)
    chip_img = np.ascontiguousarray(base[16:H + 16, 16:W + 16])
    win_img = base[16 - dv:16 - dv + H, 16 - du:16 - du + W] + rng.integers(-2, 3, (H, W)).astype(np.float32)
    win_img = np.ascontiguousarray(np.clip(win_img, 1, 255))
    cu = np.array([Dx2 // 2 + 3 + 7 * (i % 4) for i in range(12)])
    cv = np.array([Dy2 // 2 + 3 + 9 * (i // 4) for i in range(12)])
    x0, y0 = int(cu[0]) - Dx2 // 2, int(cv[0]) - Dy2 // 2

    def wnull(wx, wy):
        assert 0 <= wx < Dx2 - 1 and 0 <= wy < Dy2 - 1, (wx, wy)       # a written pixel of point 0's window
        win_img[y0 + wy, x0 + wx] = 0

    def singles(wx0):
        # x = wx0, +5, +10, +15: the four residues modulo 4; each inside the boxes of four consecutive cx of the certain set
        assert wx0 >= 14 and wx0 + 15 <= cw + 19
        for k in range(4):
            wnull(wx0 + 5 * k, 4 + (Dy2 - 10) * k // 3)

    if kind in ("single_phases", "t4_row", "both_sides"):
        singles(14)
    if kind == "t4_col":
        singles(Dx2 - 20)
    if kind == "box_sides":
        # around the box of cell (12, 2), the first pivot's start: just left of it, just right of it (the first pad byte of a row's
        # last dword when cw is no multiple of 4), the last pad byte, just above, just below; the neighbouring cells of the certain
        # set see each of them inside, outside and under a pad byte as well
        pad = (-cw) % 4
        for wx, wy in ((11, 2 + cw // 2), (12 + cw, 3 + cw // 2), (12 + cw + max(pad - 1, 0), 5 + cw // 2), (12 + cw // 3, 1), (14 + cw // 3, 2 + cw)):
            wnull(min(wx, Dx2 - 2), wy)
    if kind == "carry":
        for k, (left, right) in enumerate(NEIGHBOURS):
            wx, wy = cw // 2 + 4 + 5 * k, 5 + (Dy2 - 12) * k // 3
            wnull(wx, wy)
            win_img[y0 + wy, x0 + wx - 1] = left; win_img[y0 + wy, x0 + wx + 1] = right
    if kind == "blob_edge":
        win_img[y0:y0 + Dy2 - 1, x0:x0 + 15] = 0                       # point 0: cells cx <= 14 dirty, cx >= 15 clean
    if kind == "both_sides":
        u, v = int(cu[0]), int(cv[0])
        for dx, dy in ((2, -3), (-5, 4), (ocw, ocw), (-ocw, 0)):
            chip_img[v + dy, u + dx] = 0
        chip_img[v - 3, u + 1] = 1; chip_img[v - 3, u + 3] = 255; chip_img[v + 4, u - 6] = 128; chip_img[v + 4, u - 4] = 127
    if kind == "one_valid_limit":
        # the box of cell (12, 2): every pixel null but its centre; then nulls outside the box, column by column from the left, until
        # point 0's search area holds one invalid pixel less than the 80 % rule's first invalid count
        box = win_img[y0 + 2:y0 + 2 + cw, x0 + 12:x0 + 12 + cw]
        keep = box[cw // 2, cw // 2]
        box[:] = 0; box[cw // 2, cw // 2] = keep
        need = nc.first_invalid_count(Dx2 * Dy2) - 1 - (cw * cw - 1) - (Dx2 + Dy2 - 1)
        cols = [x for x in range(Dx2 - 1) if not 12 <= x < 12 + cw]
        for wx in cols:
            for wy in range(Dy2 - 1):
                if need > 0:
                    wnull(wx, wy); need -= 1
        assert need == 0
    if lift:
        chip_img = np.where(chip_img > 0, chip_img + lift, 0).astype(np.float32)
        win_img = np.where(win_img > 0, win_img + lift, 0).astype(np.float32)
    xy = np.zeros((12, 6))
    xy[:, 2] = cu; xy[:, 3] = cv
    xy[:, 0] = cu * synth.MPP; xy[:, 1] = -cv * synth.MPP
    return MaskCase(kind, ocw, chip_img, win_img, xy, np.zeros(2, np.int32), x0, y0)


def pivots(oracle, c):
    H, W = c.chip_img.shape
    off, uv = oracle.get_uv_pivot(c.xyuvav, 16.0, 15.0, c.ocw, H, W)
    last = uv[off[1:] - 1]
    assert (np.abs(last[:, 0]) == 10).all() and (last[:, 1] == 0).all(), "the zero velocity no longer gives pivots (0..10, 0)"
    return off, uv


def cell_kinds(c, k):
    """Counted in numpy over the certain set of point k (cells cx 11..23, cy 1..3): how many boxes are clean, how many hold a null,
    the set of (box origin phase, null phase) pairs (window x modulo 4) of the nulls inside boxes, how many (box, null) pairs have the
    null under a pad byte of a row's last dword, and how many have it one pixel outside the box on each side."""
    _, _, cw = geometry(c.ocw)
    w = c.window(k)
    u = int(c.xyuvav[k, 2])
    wx_img0 = u - geometry(c.ocw)[0] // 2                  # image x of window column 0: phases are taken on image x
    pad = (-cw) % 4
    out = dict(clean=0, dirty=0, phases=set(), pad=0, left=0, right=0, above=0, below=0, min_valid=cw * cw)
    for cy in (1, 2, 3):
        for cx in range(11, 24):
            box = w[cy:cy + cw, cx:cx + cw]
            z = np.argwhere(box == 0)
            out["clean" if len(z) == 0 else "dirty"] += 1
            out["min_valid"] = min(out["min_valid"], cw * cw - len(z))
            for zy, zx in z:
                out["phases"].add(((wx_img0 + cx) % 4, (wx_img0 + cx + zx) % 4))
            out["pad"] += int((w[cy:cy + cw, cx + cw:cx + cw + pad] == 0).sum())
            out["left"] += int((w[cy:cy + cw, cx - 1] == 0).sum())
            out["right"] += int((w[cy:cy + cw, cx + cw] == 0).sum())
            out["above"] += int((w[cy - 1, cx:cx + cw] == 0).sum())
            out["below"] += int((w[cy + cw, cx:cx + cw] == 0).sum())
    return out
