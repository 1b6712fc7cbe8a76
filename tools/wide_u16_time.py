#!/usr/bin/env python3
"""Time the exhaustive search beyond +-15 px on a scaled-integer pair on the matrix cores (mimc3_match_ncc_wide_planes) on BASELINE C2:
  python3 tools/wide_u16_time.py [--label NAME] [--out DIR] [--series ocw:R,ocw:R,...] [--npeaks 0,4] [--pairs dn12,ddx]

C2 as 12-bit DN (tests/full_chip_u16_common.spread12) and as its d/dx pair (the 8-bit pair after the program's filter 1), the points of
tools/wide_u8_time.py (C2's grid points whose chip and box at ocw 80, R 15 stay inside the image: about 189,000 of the 200,000), one
process, the configurations of a pair interleaved pass by pass, median of 3 passes after 2, with min and max.  Series: ocw 16 at
R 16 / 23 / 31 / 32 / 47; ocw 7, 40 and 80 at R 16 and at their largest R (47, 47, 27), ocw 40 also at 39, the float wide kernel's
limit there; npeaks 0 and 4.  Per configuration:
  (a) wide_planes          the new entry in mode 1: the matrix-core wide kernel on the u16 planes, both forms;
  (b) wide_planes_clean    its clean form alone (MIMC3_WIDE_U16_FORMS=1), from which the masked form's share of (a) follows;
  (c) wide                 match_ncc_wide_dev in the same session, where that entry takes (ocw, R): the float wide kernel;
  (d) chip_planes_r15      match_ncc_full_chip_planes_dev(mode 1) at R 15 and the same ocw: the unit -- the new kernel computes
                           ceil(S / 32)^2 tiles of that kernel's one.
One JSON line per configuration with every pass (device time of a whole pass, HIP events through the context's timing hooks).  `faster`
says whether EVERY pass of (a) was faster than EVERY pass of (c) -- the rule mode 0's dispatch follows.  With --out also written to
DIR/timings.jsonl and DIR/table.txt.  Test / tuning infrastructure."""
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
from full_planes_time import arg  # noqa: E402
from full_chip_u16_common import spread12  # noqa: E402

SERIES = "16:16,16:23,16:31,16:32,16:47,7:16,7:47,40:16,40:39,40:47,80:16,80:27"
HEAD = "pair  ocw  R  K   new ms (min-max)        clean ms   float ms (min-max)        float/new  unit ms  tiles  new/(tiles*unit)  LDS B   WG/CU  faster"


def run_pair(pair, c, xy, shift, series, npk, label, reps, warm):
    n = xy.shape[0]
    configs = []
    for ocw, R in series:
        for K in npk:
            configs += [("wide_planes", ocw, R, K), ("wide_planes_clean", ocw, R, K)]
            if R <= api.wide_max_radius(ocw):
                configs.append(("wide", ocw, R, K))
            if ("chip_planes_r15", ocw, 15, K) not in configs:
                configs.append(("chip_planes_r15", ocw, 15, K))
    lines, table = [], []
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out, d_cand = DevArray(src=xy), DevArray(src=shift), DevArray((n, 8), np.float32), DevArray((8, n, 3), np.float32)
        ctx.enable_timing(True)
        if pair == "dn12":
            ctx.set_images(spread12(c.i0), spread12(c.i1))
        else:
            ctx.set_images(c.i0, c.i1)
            ctx.filter_images(api.CLI_KERNELS[0])
        ms = {cfg: [] for cfg in configs}
        status = {}
        for k in range(warm + reps):
            for cfg in configs:
                entry, ocw, R, K = cfg
                cand = d_cand.ptr if K else 0
                if entry == "wide":
                    ctx.match_ncc_wide_dev(d_xy.ptr, n, c.offset, ocw, R, K, d_out.ptr, cand, d_shift=d_sh.ptr)
                    want = "f32g_wide"
                elif entry == "chip_planes_r15":
                    ctx.match_ncc_full_chip_planes_dev(d_xy.ptr, n, c.offset, ocw, R, K, d_out.ptr, cand, d_shift=d_sh.ptr, mode=1)
                    want = "u16_mfma_chip"
                else:
                    if entry == "wide_planes_clean":
                        os.environ["MIMC3_WIDE_U16_FORMS"] = "1"
                    ctx.match_ncc_wide_planes_dev(d_xy.ptr, n, c.offset, ocw, R, K, d_out.ptr, cand, d_shift=d_sh.ptr, mode=1)
                    os.environ.pop("MIMC3_WIDE_U16_FORMS", None)
                    want = "u16_mfma_wide"
                t = ctx.last_kernel_ms()
                assert ctx.last_path() == want, (cfg, ctx.last_path())
                if k >= warm:
                    ms[cfg].append(t)
                if k == warm and entry in ("wide_planes", "wide"):
                    st = d_out.numpy()[:, 2]
                    status[cfg] = {"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()), "-3": int((st == -3).sum()), "-4": int((st == -4).sum())}
        for cfg in configs:
            entry, ocw, R, K = cfg
            p = ms[cfg]
            med = float(np.median(p))
            rec = {"tree": label, "pair": pair, "entry": entry, "case": "C2", "n": n, "ocw": ocw, "radius": R, "npeaks": K, "reps": reps,
                   "pass_ms": [round(float(t), 4) for t in p], "pass_ms_median": med, "pass_ms_min": float(min(p)), "pass_ms_max": float(max(p)),
                   "ns_per_point": 1e6 * med / n}
            if cfg in status:
                rec["status"] = status[cfg]
            if entry == "wide_planes":
                kcw, ntx, nt, lds = api.wide_planes_layout(ocw, R)
                unit = float(np.median(ms[("chip_planes_r15", ocw, 15, K)]))
                cl = float(np.median(ms[("wide_planes_clean", ocw, R, K)]))
                rec.update(layout_kcw_tiles_threads_lds=[kcw, ntx, nt, lds], workgroups_per_cu_by_lds=(160 * 1024) // lds, clean_form_ms=cl,
                           masked_form_ms=med - cl, r15_pass_ms=unit, tiles=ntx * ntx, over_tiles_times_r15=med / (ntx * ntx * unit))
                flt = ms.get(("wide", ocw, R, K))
                fl_txt, ratio_txt, faster_txt = "-", "-", "only kernel"
                if flt:
                    fm = float(np.median(flt))
                    rec["float_kernel_ms"], rec["float_kernel_over_this"], rec["faster"] = fm, fm / med, bool(max(p) < min(flt))
                    if status.get(cfg) is not None and status.get(("wide", ocw, R, K)) is not None:
                        rec["same_statuses_as_float_kernel"] = status[cfg] == status[("wide", ocw, R, K)]
                    fl_txt, ratio_txt, faster_txt = "%.1f (%.1f-%.1f)" % (fm, min(flt), max(flt)), "%.1f" % (fm / med), str(rec["faster"])
                table.append("%-5s %3d %2d %2d  %8.2f (%.2f-%.2f)  %8.2f   %-24s  %8s  %7.2f  %5d  %15.2f  %6d  %5d  %s" % (
                    pair, ocw, R, K, med, min(p), max(p), cl, fl_txt, ratio_txt, unit, ntx * ntx, med / (ntx * ntx * unit), lds, (160 * 1024) // lds,
                    faster_txt))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    return lines, table


def main():
    reps, warm = 3, 2
    label, out_dir = arg("--label", "this tree"), arg("--out", "")
    series = [tuple(int(v) for v in s.split(":")) for s in arg("--series", SERIES).split(",")]
    npk = [int(v) for v in arg("--npeaks", "0,4").split(",")]
    pairs = arg("--pairs", "dn12,ddx").split(",")
    c = synth.make_case("C2")
    shift_all = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    H, W = c.i0.shape
    reach = api.full_chip_max_ocw() + 15 + 8
    u, v = c.xyuvav[:, 2], c.xyuvav[:, 3]
    keep = (u >= reach) & (u < W - reach) & (v >= reach) & (v < H - reach)
    xy, shift = np.ascontiguousarray(c.xyuvav[keep]), np.ascontiguousarray(shift_all[keep])
    lines, table = [], [HEAD]
    for pair in pairs:
        ln, tb = run_pair(pair, c, xy, shift, series, npk, label, reps, warm)
        lines += ln
        table += tb
        print("\n".join([HEAD] + tb), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "timings.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(out_dir, "table.txt"), "w") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
