#!/usr/bin/env python3
"""Time the exhaustive search on scaled-integer pairs at any chip size on the matrix cores (mimc3_match_ncc_full_chip_planes) on BASELINE C2:
  python3 tools/full_chip_u16_time.py [--label NAME] [--out DIR] [--pair dn12|ddx|both]
  python3 tools/full_chip_u16_time.py --table DIR        (no GPU: the min - max table of the series in DIR, also written to DIR/table.txt)

Two pairs: C2 as 12-bit DN with all twelve bits varying (tests/full_chip_u16_common.py spread12: a null stays 0, every other pixel p at
(x, y) becomes 16 (p - 1) + 1 + (3 x + 5 y + 7 p) mod 16 -- not the pair x 16), and C2's 8-bit pair after filter_images(d/dx).  The points of
tools/full_chip_time.py (C2's grid points whose chip and box at ocw 80, R 15 stay inside the image: about 189,000 of the 200,000), R 15,
npeaks 0, one process, the configurations interleaved pass by pass, median of 3 passes after 2:
  (a) the new entry in mode 1 at ocw 7, 10, 11, 14, 16, 30, 40, 60, 80 (the matrix-core kernel on the u16 planes, both forms);
  (b) match_ncc_full_chip_dev(mode 1) at the same ocw: the run-time-ocw float kernel, what such a call costs without the new kernel;
  (c) match_ncc_full_planes_dev at 16 and 40: the templated u16 kernel;
  (d) the clean form alone (MIMC3_CHIP_U16_FORMS=1), from which the masked form's share of (a) follows; the dirty share per ocw.
One JSON line per configuration with every pass, device time of a whole pass (HIP events through the context's timing hooks); `faster`
says whether EVERY pass of (a) was faster than EVERY pass of (b) -- the rule mode 0's dispatch follows.  With --out also written to
DIR/full_chip_u16_time_C2_<pair>.jsonl, and the table of both pairs to DIR/table.txt once both series are there.  Test / tuning
infrastructure."""
import json
import os
import sys

import numpy as np

ROOT = os.environ.get("MIMC3_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mimc3_amd import api, synth  # noqa: E402
from hipmem import DevArray  # noqa: E402
from full_planes_time import arg, dirty_share  # noqa: E402
from full_chip_u16_common import spread12  # noqa: E402

OCWS = (7, 10, 11, 14, 16, 30, 40, 60, 80)
PAIRS = {"dn12": "C2 as 12-bit DN", "ddx": "C2's 8-bit pair after filter_images(d/dx)"}


def series_file(out_dir, pair):
    return os.path.join(out_dir, f"full_chip_u16_time_C2_{pair}.jsonl")


def table(out_dir):
    """The series of DIR as text: per pair and ocw the median and the min - max of the passes of the new kernel and of the float kernel"""
    text = []
    for pair, name in PAIRS.items():
        if not os.path.exists(series_file(out_dir, pair)):
            continue
        by = {}
        for line in open(series_file(out_dir, pair)):
            r = json.loads(line)
            by[(r["entry"], r["ocw"])] = r
        text.append(f"{name} ({os.path.basename(series_file(out_dir, pair))}):\n")
        text.append("ocw   dirty share   planes ms (min - max)          clean form   masked form   full_chip ms (min - max)         "
                    "full_chip / planes   full_planes ms   planes / full_planes   faster")
        for o in OCWS:
            p, f, t = by[("planes", o)], by[("full_chip", o)], by.get(("full_planes", o))
            text.append("%3d     %.3f      %8.3f (%.3f - %.3f)      %6.3f      %8.3f      %8.2f (%.2f - %.2f)      %5.1f          %s   %s" % (
                o, p["dirty_share"], p["pass_ms_median"], min(p["pass_ms"]), max(p["pass_ms"]), p["clean_form_ms"], p["masked_form_ms"],
                f["pass_ms_median"], min(f["pass_ms"]), max(f["pass_ms"]), p["float_kernel_over_this"],
                ("%8.2f          %.3f" % (t["pass_ms_median"], p["ratio_to_templated_kernel"])) if t else " " * 26, p["faster"]))
        text.append("")
    text = "\n".join(text)
    with open(os.path.join(out_dir, "table.txt"), "w") as f:
        f.write(text)
    return text


def series(pair, c, xy, shift, label, out_dir):
    R, reps, warm = 15, 3, 2
    n = xy.shape[0]
    configs = [(e, o) for o in OCWS for e in ("planes", "planes_clean_form", "full_chip")] + [("full_planes", 16), ("full_planes", 40)]
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=xy), DevArray(src=shift), DevArray((n, 8), np.float32)
        ctx.enable_timing(True)
        if pair == "dn12":
            i0, i1 = spread12(c.i0), spread12(c.i1)
            ctx.set_images(i0, i1)
        else:
            ctx.set_images(c.i0, c.i1)
            ctx.filter_images(api.CLI_KERNELS[0])
            i0, i1 = ctx.get_images(*c.i0.shape)
        ms = {cfg: [] for cfg in configs}
        for k in range(warm + reps):
            for entry, ocw in configs:
                if entry == "full_planes":
                    ctx.match_ncc_full_planes_dev(d_xy.ptr, n, c.offset, ocw, R, 0, d_out.ptr, 0, d_shift=d_sh.ptr)
                    want = "u16_full"
                elif entry == "full_chip":
                    ctx.match_ncc_full_chip_dev(d_xy.ptr, n, c.offset, ocw, R, 0, d_out.ptr, 0, d_shift=d_sh.ptr, mode=1)
                    want = "f32g_chip"
                else:
                    if entry == "planes_clean_form":
                        os.environ["MIMC3_CHIP_U16_FORMS"] = "1"
                    ctx.match_ncc_full_chip_planes_dev(d_xy.ptr, n, c.offset, ocw, R, 0, d_out.ptr, 0, d_shift=d_sh.ptr, mode=1)
                    os.environ.pop("MIMC3_CHIP_U16_FORMS", None)
                    want = "u16_mfma_chip"
                t = ctx.last_kernel_ms()
                assert ctx.last_path() == want, (entry, ocw, ctx.last_path())
                if k >= warm:
                    ms[(entry, ocw)].append(t)
        lines = []
        for entry, ocw in configs:
            p = ms[(entry, ocw)]
            med = float(np.median(p))
            rec = {"tree": label, "pair": pair, "entry": entry, "case": "C2", "n": n, "ocw": ocw, "radius": R, "reps": reps,
                   "pass_ms": [round(float(t), 4) for t in p], "pass_ms_median": med, "ns_per_point": 1e6 * med / n}
            if entry == "planes":
                flt, cl = ms[("full_chip", ocw)], float(np.median(ms[("planes_clean_form", ocw)]))
                rec["dirty_share"] = dirty_share(i0, i1, xy, c.offset, shift, ocw, R)
                rec["layout_kcw_ntr_kcv_lds"] = api.full_chip_planes_layout(ocw)
                rec["clean_form_ms"], rec["masked_form_ms"] = cl, med - cl
                rec["float_kernel_over_this"] = float(np.median(flt)) / med
                rec["faster"] = bool(max(p) < min(flt))
                if ("full_planes", ocw) in ms:
                    rec["ratio_to_templated_kernel"] = med / float(np.median(ms[("full_planes", ocw)]))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(series_file(out_dir, pair), "w") as f:
                f.write("\n".join(lines) + "\n")


def main():
    R = 15
    if "--table" in sys.argv:
        print(table(arg("--table", ".")))
        return
    label, out_dir, which = arg("--label", "this tree"), arg("--out", ""), arg("--pair", "both")
    c = synth.make_case("C2")
    shift_all = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    H, W = c.i0.shape
    reach = api.full_chip_max_ocw() + R + 8
    u, v = c.xyuvav[:, 2], c.xyuvav[:, 3]
    keep = (u >= reach) & (u < W - reach) & (v >= reach) & (v < H - reach)
    xy, shift = np.ascontiguousarray(c.xyuvav[keep]), np.ascontiguousarray(shift_all[keep])
    for pair in ("dn12", "ddx") if which == "both" else (which,):
        series(pair, c, xy, shift, label, out_dir)
    if out_dir:
        print(table(out_dir))


if __name__ == "__main__":
    main()
