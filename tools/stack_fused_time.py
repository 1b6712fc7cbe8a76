#!/usr/bin/env python3
"""Time fused stack layers (mimc3_stack_add_fused: the accumulating forms of the run-time-ocw matrix-core searches) on BASELINE C2's pair
and grid (200,000 points, ocw 16):
  python3 tools/stack_fused_time.py [--reps 3] [--label NAME] [--pairs u8,dn12] [--radii 15,16,31,47] [--out profiles/stack_fused/stack_fused_time_C2.jsonl]
  python3 tools/stack_fused_time.py --demo

One JSON line per (pair, ocw, R), printed and appended to --out.  C2 as 8-bit and as 12-bit DN (times 16) in ONE process; per
configuration the calls are interleaved -- one round is one call of each -- and the device time of every call (HIP events through the
context's timing hooks, around the whole call) is kept: median, min and max over K rounds (default 3) after two warm-up rounds, of
  fused    stack_add_fused_dev: one launch pair over all points, the surfaces added from LDS;
  other    at R 15 stack_add_class_dev (the class kernel through the layer scratch), at R 16 / 31 / 47 stack_add_dev (the float wide
           kernel through the layer scratch) -- the layer the stack had before, with the same bytes afterwards.
On the 8-bit pair ocw 10 and 60 at R 15 as well (fused alone: no other add takes these chip sizes).
--demo prints, on the device, the misplaced-point counts of tests/test_wide_stack_cpu.py's five (34, -27) px pairs at R 40 through the
fused entry (per layer from match_ncc_wide_planes, and stacked).  Test / tuning infrastructure."""
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


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def demo():
    from stack_common import misplaced
    from test_wide_stack_cpu import FAR_STACK_OCW, FAR_STACK_R, far_series
    from wide_common import FAR_TRUE
    series = far_series()
    per_layer, paths = [], []
    with api.Context(0) as ctx:
        ctx.stack_begin_wide(series[0].n, FAR_STACK_R)
        for c in series:
            ctx.set_images(c.i0, c.i1)
            per_layer.append(int(misplaced(ctx.match_ncc_wide_planes(c.xyuvav, (0, 0), FAR_STACK_OCW, FAR_STACK_R)[0], FAR_TRUE).sum()))
            ctx.stack_add_fused(c.xyuvav, (0, 0), FAR_STACK_OCW)
            paths.append(ctx.last_path())
        stacked = int(misplaced(ctx.stack_finish()[0], FAR_TRUE).sum())
    print(json.dumps({"demo": "far series through stack_add_fused", "n": series[0].n, "ocw": FAR_STACK_OCW, "radius": FAR_STACK_R,
                      "paths": sorted(set(paths)), "misplaced_per_layer": per_layer, "misplaced_stacked": stacked}), flush=True)


def main():
    if "--demo" in sys.argv:
        return demo()
    reps = int(arg("--reps", 3))
    label = arg("--label", "this tree")
    pairs = str(arg("--pairs", "u8,dn12")).split(",")
    radii = [int(v) for v in str(arg("--radii", "15,16,31,47")).split(",")]
    out_path = arg("--out", os.path.join(ROOT, "profiles", "stack_fused", "stack_fused_time_C2.jsonl"))
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    images = {"u8": lambda: (c.i0, c.i1), "dn12": lambda: (c.i0 * 16, c.i1 * 16)}
    d_xy = DevArray(src=np.ascontiguousarray(c.xyuvav))
    with api.Context(0) as ctx:
        for pair in pairs:
            ctx.enable_timing(False)
            ctx.set_images(*images[pair]())
            configs = [(c.ocw, R) for R in radii] + ([(10, 15), (60, 15)] if pair == "u8" else [])
            for ocw, R in configs:
                ctx.enable_timing(False)
                ctx.stack_begin_wide(c.n, R, shift)
                ctx.enable_timing(True)
                calls = {"fused": lambda: ctx.stack_add_fused_dev(d_xy.ptr, c.n, c.offset, ocw)}
                if ocw == c.ocw:
                    other = "stack_add_class" if R <= 15 else "stack_add"
                    calls[other] = (lambda: ctx.stack_add_class_dev(d_xy.ptr, c.n, c.offset, ocw)) if R <= 15 else \
                                   (lambda: ctx.stack_add_dev(d_xy.ptr, c.n, c.offset, ocw))
                ms, paths = {k: [] for k in calls}, {}
                for k in range(reps + 2):                                # one round = one call of each, interleaved
                    for name, call in calls.items():
                        call()
                        t = ctx.last_kernel_ms()
                        paths[name] = ctx.last_path()
                        if k >= 2:
                            ms[name].append(t)
                st = {k: stats(v) for k, v in ms.items()}
                NC = (2 * R + 1) ** 2
                rec = {"tree": label, "entry": "stack_fused", "pair": pair, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                       "paths": paths, "fused_ms": st["fused"], "all_ms": {k: [float(v) for v in ms[k]] for k in ms},
                       "state_bytes_per_layer": 20 * c.n * NC, "layers": ctx.stack_info()[2]}
                for name in calls:
                    if name != "fused":
                        spread = max(st[name]["max"] - st[name]["min"], st["fused"]["max"] - st["fused"]["min"])
                        rec.update({"other": name, "other_ms": st[name], "speedup": st[name]["median"] / st["fused"]["median"],
                                    "faster_by_more_than_spread": bool(st[name]["median"] - st["fused"]["median"] > spread)})
                line = json.dumps(rec)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "a") as f:
                    f.write(line + "\n")
            ctx.enable_timing(False)
            ctx.stack_begin_wide(0, 0)                                   # (release the state before the next pair)


if __name__ == "__main__":
    main()
