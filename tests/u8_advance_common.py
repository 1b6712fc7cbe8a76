"""Test infrastructure of the u8 step's advance list (mx_climb_area, match_kernel.h; u8_classify_kernel.hip): the rule restated in
numpy, the small fixtures, and the list figures of the MIMC3_MX_STATS lines read from a child process -- shared by
tests/test_u8_advance_cpu.py and tests/test_u8_advance.py."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np

from conftest import ROOT
from mimc3_amd import synth

GROW = 2            # kMxAreaGrow
BORDER = 256        # the planes' zero border: what lies outside the image is null


def axis_geometry(l, ocw):
    """one axis of mx_tile_fit and mx_climb_area for last-pivot components l (array): (fits, tile origin, first and last cell of
    the climb area as window cells, first pixel and pixel count of the area's boxes clipped to the written area)"""
    l = np.asarray(l, np.int64)
    d2 = np.abs(l) + ocw + 2
    cs = 2 * d2 + 1 - 2 * ocw + 1
    c0, c1 = d2 - ocw, d2 - ocw + l
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    big = cs - 2 > 32
    t0b = np.minimum(np.maximum((lo + hi) // 2 - 15, 1), cs - 2 - 31)          # (lo + hi > 0: floor = C's truncation)
    fits = np.where(big, (lo - 1 >= t0b) & (hi + 1 <= t0b + 31), True)
    t0 = np.where(big, t0b, 1)
    a0 = np.maximum(np.maximum(lo - GROW, 1), t0)
    a1 = np.minimum(np.minimum(hi + GROW, cs - 2), t0 + 31)
    npx = np.minimum(a1 + 2 * ocw + 1, 2 * d2) - a0
    return fits, t0, a0, a1, a0, npx


def null_table(img):
    """summed-area table of the null mask of the zero-bordered plane (the border is null)"""
    H, W = img.shape
    z = np.ones((H + 2 * BORDER + 1, W + 2 * BORDER + 1), np.int64)
    z[0, :] = 0
    z[:, 0] = 0
    z[BORDER + 1:BORDER + H + 1, BORDER + 1:BORDER + W + 1] = (img == 0)
    return z.cumsum(0).cumsum(1)


def box(S, x, y, w, h):
    x, y = x + BORDER, y + BORDER
    return S[y + h, x + w] - S[y, x + w] - S[y + h, x] + S[y, x]


def classify(i0, i1, xy, offset, off, uv, ocw, swap=False):
    """dict of per-point arrays: clean (class 0), wn (window nulls only, takeable), advance (on the advance list), and the area's
    window-pixel rectangle (ax, ay, aw, ah: image coordinates of its first pixel, size) -- the rule of u8_classify restated"""
    chip, win = (i1, i0) if swap else (i0, i1)
    Sc, Sw = null_table(chip), null_table(win)
    off = np.asarray(off, np.int64)
    npiv = np.diff(off)
    last = np.asarray(uv)[off[1:] - 1].astype(np.int64)
    u0, v0 = xy[:, 2].astype(np.int64), xy[:, 3].astype(np.int64)
    fx, _, _, _, px, pw = axis_geometry(last[:, 0], ocw)
    fy, _, _, _, py, ph = axis_geometry(last[:, 1], ocw)
    dx2, dy2 = np.abs(last[:, 0]) + ocw + 2, np.abs(last[:, 1]) + ocw + 2
    wu, wv = u0 + int(offset[0]) - dx2, v0 + int(offset[1]) - dy2
    chip_n = box(Sc, u0 - ocw, v0 - ocw, 2 * ocw + 1, 2 * ocw + 1)
    win_n = box(Sw, wu, wv, 2 * dx2, 2 * dy2)
    area_n = box(Sw, wu + px, wv + py, pw, ph)
    takes = (npiv >= 1) & (npiv <= 64) & fx & fy
    wn = takes & (chip_n == 0) & (win_n > 0)
    return dict(clean=takes & (chip_n == 0) & (win_n == 0), wn=wn, advance=wn & (area_n == 0), takes=takes, chip_n=chip_n, win_n=win_n,
                ax=wu + px, ay=wv + py, aw=pw, ah=ph, wu=wu, wv=wv, dx2=dx2, dy2=dy2)


def small(ocw, seed, **kw):
    """a pair of about (2 ocw + 230)^2 pixels with 30 points (tests/test_u8_step_lists.py's)"""
    kw.setdefault("h", 2 * ocw + 230)
    kw.setdefault("w", 2 * ocw + 240)
    kw.setdefault("dimx", 6)
    kw.setdefault("dimy", 5)
    kw.setdefault("null_frac", 0.0)
    return synth.make_small(seed=seed, ocw=ocw, shift=kw.pop("shift", (3, -2)), angle_deg=kw.pop("angle_deg", 40.0),
                            speed=kw.pop("speed", 1700.0), noise_dn=2, **kw)


def pivots(api, c, ocw):
    H, W = c.i0.shape
    return api.get_uv_pivot(c.xyuvav, c.dt, c.mpp, ocw, H, W)


BORDER_SPOTS = ("out_left", "out_right", "out_top", "out_bottom", "out_tl", "out_tr", "out_bl", "out_br",
                "in_left", "in_right", "in_top", "in_bottom")


def border_case(api, ocw, spot, flip=False, g=14):
    """a null-free pair with ONE null planted in the window image, one pixel outside (out_*: sides and corners) or just inside
    (in_*: sides) the pixel rectangle of point g's climb area; the points whose window holds the null, and g.  On the last pivot's side
    the area ends at the edge of the written window, so a spot outside it there is no window pixel (second value False): `flip` turns
    the flow round, and between the two directions every spot exists.  Returns (case, spot is a written window pixel of g, g's new index)"""
    c = small(ocw, 8800 + ocw, angle_deg=140.0 if flip else 40.0, shift=(-3, -2) if flip else (3, -2))      # (the shift lies inside the corridor)
    off, uv = pivots(api, c, ocw)
    k = classify(c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw)
    assert k["clean"].all()
    ax, ay, aw, ah = (int(k[n][g]) for n in ("ax", "ay", "aw", "ah"))
    mx, my = ax + aw // 2, ay + ah // 2
    x, y = dict(out_left=(ax - 1, my), out_right=(ax + aw, my), out_top=(mx, ay - 1), out_bottom=(mx, ay + ah),
                out_tl=(ax - 1, ay - 1), out_tr=(ax + aw, ay - 1), out_bl=(ax - 1, ay + ah), out_br=(ax + aw, ay + ah),
                in_left=(ax, my), in_right=(ax + aw - 1, my), in_top=(mx, ay), in_bottom=(mx, ay + ah - 1))[spot]
    i1 = c.i1.copy()
    i1[y, x] = 0.0
    inside_window = k["wu"][g] <= x < k["wu"][g] + 2 * k["dx2"][g] and k["wv"][g] <= y < k["wv"][g] + 2 * k["dy2"][g]
    k = classify(c.i0, i1, c.xyuvav, c.offset, off, uv, ocw)
    keep = np.flatnonzero((k["win_n"] > 0) | (np.arange(len(off) - 1) == g))
    xy = np.ascontiguousarray(c.xyuvav[keep])
    uvs = [uv[off[i]:off[i + 1]] for i in keep]
    off2 = np.zeros(len(keep) + 1, np.int64)
    off2[1:] = np.cumsum([len(p) for p in uvs])
    return (c.i0, i1, xy, c.offset, off2, np.ascontiguousarray(np.concatenate(uvs), np.int32), ocw), bool(inside_window), int(np.flatnonzero(keep == g)[0])


def t4_case(api, ocw):
    """fast points (|last pivot| 12 to 20: a cell grid wider than the tile in neither axis) on a pair with blobs of nulls: areas that end
    at the last reachable cells on the far side, where the closed-form T4 terms apply, with nulls elsewhere in the window"""
    c = small(ocw, 8830 + ocw, null_frac=0.012, speed=2100.0, angle_deg=-35.0, shift=(3, 2), h=2 * ocw + 260, w=2 * ocw + 270, dimx=8, dimy=7, margin=ocw + 45)
    off, uv = pivots(api, c, ocw)
    return c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw


def blobs_case(api, ocw, seed=8860, null_frac=0.02, **kw):
    """the plain mixed case: blobs of nulls in both images"""
    c = small(ocw, seed + ocw, null_frac=null_frac, **kw)
    off, uv = pivots(api, c, ocw)
    return c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw


def off_corridor_case(api, ocw):
    """tests/test_u8_step_lists.py's off-corridor fixture (17 to 29 pivots and a shift far off the corridor: climbs leave the area and
    the tile), at ocw 16 with fewer nulls, so that several windows hold theirs outside the area"""
    c = small(ocw, 8450 + ocw, null_frac=0.03 if ocw < 16 else 0.006, shift=(9, 7), angle_deg=45.0, speed=2900.0, h=2 * ocw + 300, w=2 * ocw + 310,
              dimx=6, dimy=6, margin=ocw + 80)
    off, uv = pivots(api, c, ocw)
    assert 15 <= int(np.abs(uv[off[1:] - 1]).max()) <= 29
    return c.i0, c.i1, c.xyuvav, c.offset, off, uv, ocw


ADV_RE = r"lists clean (\d+) rest (\d+)\n.*?clean: (\d+) points staged[^\n]*rest (\d+)\n[^\n]*advance: list (\d+) tried (\d+) finished (\d+)"


def advance_stats(body, env=None, outdir=None):
    """run `body` (which defines `cases`, a list of (i0, i1, xy, offset, off, uv, ocw)) in a child process with the kernels' diagnostics
    on, one forward call per case on one context: per call (clean list, rest list, clean points finished, kMxRest afterwards, advance
    list, tried, finished); with `outdir`, call i's output goes to outdir/i.npy"""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
        import numpy as np
        from mimc3_amd import api, synth
        import u8_advance_common as ac
        %s
        outdir = %r
        if outdir:
            import os
            os.makedirs(outdir, exist_ok=True)
        with api.Context(0) as ctx:
            for i, (i0, i1, xy, offset, off, uv, ocw) in enumerate(cases):
                ctx.set_images(i0, i1)
                out = ctx.matching_ncc_dlc_2(xy, offset, off, uv, ocw)
                assert ctx.last_path() == "u8_mfma"
                if outdir:
                    np.save(os.path.join(outdir, "%%d.npy" %% i), out)
    """) % (ROOT, ROOT, body, outdir)
    e = dict(os.environ, MIMC3_MX_STATS="1")
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(ADV_RE, r.stderr, re.S)
    assert found, r.stderr[-2000:]
    return [tuple(int(v) for v in m) for m in found]
