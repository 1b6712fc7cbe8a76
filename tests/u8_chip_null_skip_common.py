"""Test infrastructure: 33-pixel 8-bit chips whose nulls sit where the chip-null skip of the register-tiled kernel can go wrong
(match_px_kernel.hip: the flag mask, PxU8::cn_task, the XYC and WNC bodies), and the numpy restatement of the mask and of both bodies.

Geometry is that of tests/u8_dirty_masks_common.py at ocw 16: a dozen points of zero velocity, pivots (0, 0) .. (10, 0), the certain
set cx 11 .. 23, cy 1 .. 3.  Chip coordinates (row, column) below are those of point 0's chip; the points are 7 px / 9 px apart, so the
other points see the same nulls at other places of their chips.

The chip of ocw 16 lives in 16 lanes: lane l owns rows l and l + 16 as nine dwords each -- task index t = 9 * half + column for
t = 0 .. 17 -- and lanes 0 .. 8 own the nine dwords of row 32 (t = 18, the tail task).  Chip column 32 is the single valid byte of a
row's last dword."""
import numpy as np

import null_encoding_common as nc
import u8_dirty_masks_common as dm

OCW, CW, GPR, NT = 16, 33, 9, 19
NPX = CW * CW
ONES = np.uint32(0x01010101)
LASTFF = np.uint32(0x000000FF)
EXTREME = (1, 127, 128, 255)

# name -> the task indices point 0's chip must flag (None: counted otherwise in the CPU test)
SINGLES = {f"single_h{h}_p{p}": {9 * h + 3} for h in (0, 1) for p in range(4)}
KINDS = dict(SINGLES, tail_lane0={18}, tail_last={18}, col32={8}, all_flagged=set(range(NT)), disc=None, coincident=None,
             extreme_bytes=None, limit_at=None, limit_short=None)
T4_KINDS = ("t4_row", "t4_col")
WINDOWS = ("clean", "dirty")          # no window null at all (XYC, clean list) / the four single window nulls of dm's "single_phases" (WNC)
COINC = ((10, 10), (20, 21), (32, 5), (3, 32))            # chip nulls of "coincident" / "extreme_bytes"
COINC_CELLS = ((10, 2), (12, 2), (22, 1))                 # cells whose window holds a null under chip null k (k = 0, 1, 2); the surface
                                                          # peaks on (10, 2), so that cell and its four neighbours all enter the fit


def chip_nulls(kind):
    """(row, column) of the nulls of point 0's chip."""
    if kind in SINGLES:
        h, p = int(kind[8]), int(kind[11])
        return [(5 + 16 * h, 12 + p)]
    if kind == "tail_lane0":
        return [(32, 1)]
    if kind == "tail_last":
        return [(32, 32)]
    if kind == "col32":
        return [(5, 32)]
    if kind == "all_flagged":         # two diagonals, one per row half, a null in every dword column of each; one in the tail row
        return [(16 * h + j, min(4 * j + j % 4, 32)) for h in (0, 1) for j in range(GPR)] + [(32, 7)]
    if kind in ("disc",) + T4_KINDS:
        return [(r, c) for r in range(CW) for c in range(CW) if (r - 16) ** 2 + (c - 14) ** 2 <= 81]
    if kind in ("coincident", "extreme_bytes"):
        return list(COINC)
    if kind in ("limit_at", "limit_short"):
        # the most nulls the 80 % rule lets pass, and one more (the point is invalid); the centre stays valid
        need = nc.first_invalid_count(NPX) - (1 if kind == "limit_at" else 0)
        return [(r, c) for c in range(CW) for r in range(CW) if (r, c) != (16, 16)][:need]
    raise KeyError(kind)


def make_case(kind, window="clean"):
    c = dm.make_case(OCW, kind if kind in T4_KINDS else "single_phases")
    if kind not in T4_KINDS and window == "clean":
        c.win_img[c.win_img == 0] = 97
    u, v = c.xyuvav[0, 2:4].astype(int)
    for r, col in chip_nulls(kind):
        c.chip_img[v - OCW + r, u - OCW + col] = 0
    if kind == "coincident":
        # cell (cx, cy) lays chip pixel (r, col) on window pixel (cx + col, cy + r): a window null there coincides with the chip's
        # null in that cell and lies one pixel left / right / above / below it in the cell's four neighbours
        for (r, col), (cx, cy) in zip(COINC, COINC_CELLS):
            c.win_img[c.y0 + cy + r, c.x0 + cx + col] = 0
    if kind == "extreme_bytes":
        # under every chip null, in every cell of the certain set and of the peak's 3 x 3 (cx 9 .. 11): window bytes 1, 127, 128, 255
        for k, (r, col) in enumerate(COINC):
            for cy in (1, 2, 3):
                for cx in range(9, 24):
                    y, x = c.y0 + cy + r, c.x0 + cx + col
                    if c.win_img[y, x] != 0:
                        c.win_img[y, x] = EXTREME[(cx + cy + k) % 4]
    return c


# ---- the kernel's view of a cell, restated ----------------------------------------------------------------------------------------
def pack(rows):
    """[33][36] bytes -> [33][9] little-endian dwords."""
    b = np.asarray(rows, np.uint32).reshape(CW, GPR, 4)
    return b[:, :, 0] | (b[:, :, 1] << np.uint32(8)) | (b[:, :, 2] << np.uint32(16)) | (b[:, :, 3] << np.uint32(24))


def chip_dwords(chip):
    """The chip in registers: its pad bytes (columns 33 .. 35 of a row's last dword) are 0."""
    a = np.zeros((CW, 4 * GPR), np.uint32)
    a[:, :CW] = chip
    return pack(a)


def window_dwords(win, cx, cy, fill):
    """What the aligned window reads of cell (cx, cy) deliver: the last dword of a row carries three window bytes from beyond the
    box (`fill` where the fixture's window ends: the LDS row goes on)."""
    w = np.full((win.shape[0], win.shape[1] + 4), fill, np.uint32)
    w[:, :win.shape[1]] = win
    return pack(w[cy:cy + CW, cx:cx + 4 * GPR])


def tasks(d):
    """[33][9] dwords -> [19][16]: task index x lane.  Tail lanes 9 .. 15 hold a zero dword (valid: False)."""
    out = np.zeros((NT, 16), np.uint32)
    pff = np.zeros((NT, 16), np.uint32)
    for h in (0, 1):
        for j in range(GPR):
            out[9 * h + j] = d[16 * h:16 * h + 16, j]
            pff[9 * h + j] = LASTFF if j == GPR - 1 else np.uint32(0xFFFFFFFF)
    out[18, :GPR] = d[32]
    pff[18, :GPR - 1] = np.uint32(0xFFFFFFFF); pff[18, GPR - 1] = LASTFF
    return out, pff


def maybe_excl(v, keep):
    """PxU8::maybe_excl: the zero-byte detector under a keep mask."""
    v = np.asarray(v, np.uint32)
    return ((v - ONES) & ~v & np.uint32(0x80808080) & keep) != 0


def flag_mask(chip):
    """The kernel's 19 ballots."""
    a, pff = tasks(chip_dwords(chip))
    return {t for t in range(NT) if maybe_excl(a[t], pff[t]).any()}


def flag_mask_plain(chip):
    """The definition: index t is flagged iff a chip pixel of its dwords is null."""
    z = np.asarray(chip) == 0
    out = {9 * h + j for h in (0, 1) for j in range(GPR) if z[16 * h:16 * h + 16, 4 * j:4 * j + 4].any()}
    return out | ({18} if z[32].any() else set())


def popc(v):
    return np.array([bin(int(x)).count("1") for x in np.asarray(v).reshape(-1)], np.int64).reshape(np.shape(v))


def body(chip, win, cx, cy, dirty, mask=None, fill=0xA5, drop_j=False, pad_nulls=False):
    """The six sums of cell (cx, cy) as the XYC (dirty False) / WNC (dirty True) body and its finish form them.  `mask`: the flag
    mask (default: the chip's).  drop_j / pad_nulls: the value-only mutations the GPU tests are run against."""
    a, pff = tasks(chip_dwords(chip))
    bw, _ = tasks(window_dwords(win, cx, cy, fill))
    bw[18, GPR:] = np.uint32(fill) * ONES                       # (the idle tail lanes read a window dword too)
    mask = flag_mask(chip) if mask is None else mask
    box = np.asarray(win[cy:cy + CW, cx:cx + CW], np.int64)
    exc = int((np.asarray(chip) == 0).sum())
    sxy = int(dm.dot4(a, bw).sum())
    csy = csyy = j8 = 0
    for t in sorted(mask):
        za = ~dm.nzff(a[t]) & (np.where(pff[t] != 0, np.uint32(0xFFFFFFFF), np.uint32(0)) if pad_nulls else pff[t])
        bz = bw[t] & za
        csy += int(dm.dot4(bz, ONES).sum()); csyy += int(dm.dot4(bz, bw[t]).sum())
        j8 += int((popc(za & ~dm.nzff(bw[t])) >> 3).sum())      # eight per pixel, shifted once per lane
    sy, syy = int(box.sum()) - csy, int((box * box).sum()) - csyy
    if not dirty:
        c = np.asarray(chip, np.int64)
        return dict(n=NPX - exc, sx=int(c.sum()), sy=sy, sxx=int((c * c).sum()), syy=syy, sxy=sxy)
    am = a & dm.nzff(bw)
    n = NPX - exc - int((box == 0).sum()) + (0 if drop_j else j8)
    return dict(n=n, sx=int(dm.dot4(am, ONES).sum()), sy=sy, sxx=int(dm.dot4(am, a).sum()), syy=syy, sxy=sxy, J=j8)


def plain(chip, win, cx, cy):
    """The NCC loop's sums: a pixel takes part iff it is non-null on both sides."""
    x = np.asarray(chip, np.int64)
    y = np.asarray(win[cy:cy + CW, cx:cx + CW], np.int64)
    ok = (x != 0) & (y != 0)
    x, y = x[ok], y[ok]
    return dict(n=int(ok.sum()), sx=int(x.sum()), sy=int(y.sum()), sxx=int((x * x).sum()), syy=int((y * y).sum()), sxy=int((x * y).sum()))


def certain_cells():
    return [(cx, cy) for cy in (1, 2, 3) for cx in range(11, 24)]
