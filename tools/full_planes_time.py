#!/usr/bin/env python3
"""Time the exhaustive search on the planes the context matches on (mimc3_match_ncc_full_planes) on BASELINE C2's pair and grid:
  python3 tools/full_planes_time.py [--reps K] [--label NAME] [--ocw 16,40]

One JSON line per run: the device time of a whole 200,000-point pass (HIP events through the context's timing hooks) -- median, mean,
min and max over K passes (default 20) after two warm-up passes:
  u8      the 8-bit pair through mimc3_match_ncc_full and, where the tree has it, through the new entry (the same kernels);
  gx      the pair after filter_images(d/dx) through the new entry, npeaks 0, with the share of points without / with nulls (host count);
  dn12    the pair times 16 (12-bit DN) through the new entry, npeaks 0 and 4.
A tree without the new entry (MIMC3_TREE = the parent commit's build) gives the u8 line of the old entry alone: run it in the same
session for the baseline and its run-to-run spread.  Test / tuning infrastructure."""
import json
import os
import sys

import numpy as np

ROOT = os.environ.get("MIMC3_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from mimc3_amd import api, synth  # noqa: E402
from hipmem import DevArray  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def dirty_share(i0, i1, xy, off, shift, ocw, R):
    """Share of the points with a null in the chip or in the search box (pixels outside the image are nulls)."""
    H, W = i0.shape
    pad = ocw + R + 1 + int(np.abs(shift).max()) + int(np.abs(np.asarray(off)).max())

    def table(img):
        z = np.pad((img == 0).astype(np.int64), pad, constant_values=1)
        return np.pad(z.cumsum(0).cumsum(1), ((1, 0), (1, 0)))

    def box(t, x0, y0, w):
        x0 = x0 + pad; y0 = y0 + pad
        return t[y0 + w, x0 + w] - t[y0, x0 + w] - t[y0 + w, x0] + t[y0, x0]

    u, v = xy[:, 2].astype(np.int64), xy[:, 3].astype(np.int64)
    cw = 2 * ocw + 1
    chip = box(table(i0), u - ocw, v - ocw, cw)
    h = ocw + R
    win = box(table(i1), u + off[0] + shift[:, 0] - h, v + off[1] + shift[:, 1] - h, 2 * h + 1)
    return float(((chip > 0) | (win > 0)).mean())


def main():
    R, reps = 15, int(arg("--reps", 20))
    ocws = [int(v) for v in str(arg("--ocw", "16,40")).split(",") if v]
    label = arg("--label", "this tree")
    c = synth.make_case("C2")
    H, W = c.i0.shape
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    planes = hasattr(api.Context, "match_ncc_full_planes_dev")
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        d_cand = DevArray((4, c.n, 3), np.float32)
        ctx.enable_timing(True)

        def report(pair, entry, ocw, npk, call, **extra):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            rec = {"tree": label, "pair": pair, "entry": entry, "npeaks": npk, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                   "path": ctx.last_path(), "pass_ms_median": float(np.median(ms)), "pass_ms_mean": float(np.mean(ms)),
                   "pass_ms_min": float(np.min(ms)), "pass_ms_max": float(np.max(ms)), "ns_per_point": 1e6 * float(np.median(ms)) / c.n}
            rec.update(extra)
            print(json.dumps(rec), flush=True)

        def new_entry(ocw, npk):
            return lambda: ctx.match_ncc_full_planes_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr if npk else 0,
                                                         d_shift=d_sh.ptr)

        for ocw in ocws:
            ctx.set_images(c.i0, c.i1)
            report("u8", "match_ncc_full", ocw, 0, lambda: ctx.match_ncc_full_dev(d_xy.ptr, c.n, c.offset, ocw, R, d_out.ptr, d_shift=d_sh.ptr))
            if not planes:
                continue
            report("u8", "match_ncc_full_planes", ocw, 0, new_entry(ocw, 0))
            ctx.filter_images(api.CLI_KERNELS[0])
            f0, f1 = ctx.get_images(H, W)
            report("gx", "match_ncc_full_planes", ocw, 0, new_entry(ocw, 0),
                   dirty_share=dirty_share(f0, f1, c.xyuvav, c.offset, shift, ocw, R))
            ctx.filter_images(None)
            i0, i1 = c.i0 * 16, c.i1 * 16
            ctx.set_images(i0, i1)
            ds = dirty_share(i0, i1, c.xyuvav, c.offset, shift, ocw, R)
            for npk in (0, 4):
                report("dn12", "match_ncc_full_planes", ocw, npk, new_entry(ocw, npk), dirty_share=ds)


if __name__ == "__main__":
    main()
