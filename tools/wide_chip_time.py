#!/usr/bin/env python3
"""Time the exhaustive search beyond +-15 px on any pair at any chip size (mimc3_match_ncc_wide_chip, match_wide_chip_kernel.hip) on
BASELINE C2:
  python3 tools/wide_chip_time.py [--label NAME] [--out DIR] [--series ocw:R,...] [--npeaks 0,4] [--pairs dn16,float] [--every K]

C2 as 16-bit DN (tests/full_dn_common.to_dn16) and as floats (tools/pyramid_any_time.as_float), the points of tools/wide_u8_time.py (C2's
grid points whose chip and box at ocw 80, R 15 stay inside the image: about 189,000 of the 200,000; --every K keeps every K-th of them
and says so in every line), one process, the configurations of a pair interleaved pass by pass so that the series alternate, median of
3 passes after 2, with min and max.  Series: ocw 10 / 16 / 40 / 80 at R 16 / 31 / 47; npeaks 0 and 4.  Per configuration:
  (a) wide_chip        the new entry in mode 1: the run-time-ocw wide float kernel;
  (b) wide             match_ncc_wide_dev in the same session, wherever that entry takes (ocw, R): the templated wide float kernel -- the
                       yardstick at the six chip sizes;
  (c) chip_r15         match_ncc_full_chip_dev(mode 1) at R 15 and the same ocw; `expected_ms` is its median times (2R + 1)^2 / 961, the
                       cell count's scale.
One JSON line per configuration with every pass (device time of a whole pass, HIP events through the context's timing hooks).  `faster`
says whether EVERY pass of (a) was faster than EVERY pass of (b).  No ratio is fixed in advance.  With --out also written to
DIR/timings.jsonl and DIR/table.txt (profiles/full_search_wide_chip/).  Test / tuning infrastructure."""
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
from full_dn_common import to_dn16  # noqa: E402
from pyramid_any_time import arg, as_float  # noqa: E402

SERIES = ",".join(f"{o}:{r}" for o in (10, 16, 40, 80) for r in (16, 31, 47))
HEAD = "pair   ocw  R  K   new ms (min-max)            templated ms (min-max)      templated/new  R15 ms  expected ms  new/expected  tiles bands  LDS B  WG/CU  faster"


def run_pair(pair, c, xy, shift, series, npk, label, reps, warm, every):
    n = xy.shape[0]
    configs = []
    for ocw, R in series:
        for K in npk:
            configs.append(("wide_chip", ocw, R, K))
            if R <= api.wide_max_radius(ocw):
                configs.append(("wide", ocw, R, K))
            if ("chip_r15", ocw, 15, K) not in configs:
                configs.append(("chip_r15", ocw, 15, K))
    lines, table = [], []
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out, d_cand = DevArray(src=xy), DevArray(src=shift), DevArray((n, 8), np.float32), DevArray((8, n, 3), np.float32)
        ctx.enable_timing(True)
        if pair == "dn16":
            ctx.set_images(to_dn16(c.i0, 5), to_dn16(c.i1, 6))
        else:
            ctx.set_images(as_float(c.i0, 5), as_float(c.i1, 6))
        ms = {cfg: [] for cfg in configs}
        status = {}
        for k in range(warm + reps):
            print(f"{pair}: pass {k + 1} of {warm + reps}", file=sys.stderr, flush=True)
            for cfg in configs:
                entry, ocw, R, K = cfg
                cand = d_cand.ptr if K else 0
                if entry == "wide":
                    ctx.match_ncc_wide_dev(d_xy.ptr, n, c.offset, ocw, R, K, d_out.ptr, cand, d_shift=d_sh.ptr)
                    want = "f32g_wide"
                elif entry == "chip_r15":
                    ctx.match_ncc_full_chip_dev(d_xy.ptr, n, c.offset, ocw, R, K, d_out.ptr, cand, d_shift=d_sh.ptr, mode=1)
                    want = "f32g_chip"
                else:
                    ctx.match_ncc_wide_chip_dev(d_xy.ptr, n, c.offset, ocw, R, K, d_out.ptr, cand, d_shift=d_sh.ptr, mode=1)
                    want = "f32g_wide_chip"
                t = ctx.last_kernel_ms()
                assert ctx.last_path() == want, (cfg, ctx.last_path())
                if k >= warm:
                    ms[cfg].append(t)
                if k == warm and entry in ("wide_chip", "wide"):
                    st = d_out.numpy()[:, 2]
                    status[cfg] = {"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()), "-3": int((st == -3).sum()), "-4": int((st == -4).sum())}
        for cfg in configs:
            entry, ocw, R, K = cfg
            p = ms[cfg]
            med = float(np.median(p))
            rec = {"tree": label, "pair": pair, "entry": entry, "case": "C2", "n": n, "every": every, "ocw": ocw, "radius": R, "npeaks": K,
                   "reps": reps, "pass_ms": [round(float(t), 4) for t in p], "pass_ms_median": med, "pass_ms_min": float(min(p)),
                   "pass_ms_max": float(max(p)), "ns_per_point": 1e6 * med / n}
            if cfg in status:
                rec["status"] = status[cfg]
            if entry == "wide_chip":
                ntx, br, nb, wgs, lds = api.wide_chip_layout(ocw, R)
                unit = float(np.median(ms[("chip_r15", ocw, 15, K)]))
                exp = unit * (2 * R + 1) ** 2 / 961.0
                rec.update(layout_tiles_bandrows_bands_wgs_lds=[ntx, br, nb, wgs, lds], r15_pass_ms=unit, expected_ms=exp, over_expected=med / exp)
                old = ms.get(("wide", ocw, R, K))
                o_txt, ratio_txt, faster_txt = "-", "-", "only kernel"
                if old:
                    om = float(np.median(old))
                    rec["templated_kernel_ms"], rec["templated_over_this"], rec["faster"] = om, om / med, bool(max(p) < min(old))
                    if status.get(cfg) is not None and status.get(("wide", ocw, R, K)) is not None:
                        rec["same_statuses_as_templated_kernel"] = status[cfg] == status[("wide", ocw, R, K)]
                    o_txt, ratio_txt, faster_txt = "%.1f (%.1f-%.1f)" % (om, min(old), max(old)), "%.2f" % (om / med), str(rec["faster"])
                table.append("%-6s %3d %2d %2d  %9.2f (%.2f-%.2f)  %-26s  %12s  %7.2f  %10.2f  %11.2f  %5d %5d  %6d  %5d  %s" % (
                    pair, ocw, R, K, med, min(p), max(p), o_txt, ratio_txt, unit, exp, med / exp, ntx * ntx, nb, lds, wgs, faster_txt))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    return lines, table


def main():
    reps, warm = 3, 2
    label, out_dir = arg("--label", "this tree"), arg("--out", "")
    series = [tuple(int(v) for v in s.split(":")) for s in arg("--series", SERIES).split(",")]
    npk = [int(v) for v in arg("--npeaks", "0,4").split(",")]
    pairs = arg("--pairs", "dn16,float").split(",")
    every = int(arg("--every", "1"))
    c = synth.make_case("C2")
    shift_all = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    H, W = c.i0.shape
    reach = api.full_chip_max_ocw() + 15 + 8
    u, v = c.xyuvav[:, 2], c.xyuvav[:, 3]
    keep = (u >= reach) & (u < W - reach) & (v >= reach) & (v < H - reach)
    xy, shift = np.ascontiguousarray(c.xyuvav[keep][::every]), np.ascontiguousarray(shift_all[keep][::every])
    lines, table = [], [HEAD]
    for pair in pairs:
        ln, tb = run_pair(pair, c, xy, shift, series, npk, label, reps, warm, every)
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
