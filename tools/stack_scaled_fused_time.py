#!/usr/bin/env python3
"""Time fused SCALED stack layers (mimc3_stack_add_scaled_fused: the scaled accumulating form of the run-time-ocw matrix-core searches)
on BASELINE C2's pair and grid (200,000 points, ocw 16), stack R 15:
  python3 tools/stack_scaled_fused_time.py [--reps 3] [--label NAME] [--pairs u8,dn12] [--out profiles/stack_scaled_fused/stack_scaled_fused_time_C2.jsonl]
  python3 tools/stack_scaled_fused_time.py --demo

One JSON line per (pair, ocw, scale), printed and appended to --out.  C2 as 8-bit and as 12-bit DN (times 16) in ONE process; per
configuration the calls are interleaved -- one round is one call of each -- and the device time of every call (HIP events through the
context's timing hooks, around the whole call) is kept: median, min and max over K rounds (default 3) after two warm-up rounds, of
  scale 1   fused_scaled   stack_add_scaled_fused_dev at scale 1, weight 1, layer radius 15 (the resampling loop on integer taps)
            stack_add_fused   stack_add_fused_dev: the same bytes through the unscaled accumulating form
  scale 2   fused_scaled   stack_add_scaled_fused_dev at layer radius 31: one launch pair, every surface resampled from LDS
            stack_add_scaled   stack_add_scaled_dev with the same arguments: the float wide kernel through the layer scratch in chunks
            search   the search alone at R 31 around the layer shift, record only: match_ncc_wide_class_dev on the 8-bit pair,
                     match_ncc_wide_planes_dev on the 12-bit one
On the 8-bit pair ocw 10 and 60 at scale 2 as well (fused alone: no other scaled add takes these chip sizes).
--demo prints, on the device, the misplaced-point counts of tests/test_stack_scaled_cpu.py's series over six time baselines stacked
through the new entry at ocw 10, a chip size no other scaled add takes (per layer from match_ncc_wide_planes, the scaled stack, the
unscaled stack through stack_add_fused).  Test / tuning infrastructure."""
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

DEMO_OCW = 10


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def demo():
    from full_fb_common import FB_OFFSET, fb_points
    from stack_common import misplaced
    from stack_scaled_common import SCALED_MOTION, SCALED_R, layer_truth, scaled_series_pairs
    xy, shift = fb_points(ocw=DEMO_OCW, radius=SCALED_R)
    per_layer, scales, paths = [], [], []
    with api.Context(0) as ctx, api.Context(0) as plain:
        ctx.stack_begin(xy.shape[0], SCALED_R, shift)
        plain.stack_begin(xy.shape[0], SCALED_R, shift)
        for s, i0, i1 in scaled_series_pairs():
            ctx.set_images(i0, i1)
            plain.set_images(i0, i1)
            rec = ctx.match_ncc_wide_planes(xy, FB_OFFSET, DEMO_OCW, api.stack_layer_radius(SCALED_R, s), shift=ctx.stack_layer_shift(s))[0]
            per_layer.append(int(misplaced(rec, layer_truth(s)).sum()))
            scales.append(s)
            ctx.stack_add_scaled_fused(xy, FB_OFFSET, DEMO_OCW, s)
            paths.append(ctx.last_path())
            plain.stack_add_fused(xy, FB_OFFSET, DEMO_OCW)
        stacked = int(misplaced(ctx.stack_finish()[0], SCALED_MOTION).sum())
        unscaled = int(misplaced(plain.stack_finish()[0], SCALED_MOTION).sum())
    print(json.dumps({"demo": "six time baselines through stack_add_scaled_fused", "n": int(xy.shape[0]), "ocw": DEMO_OCW, "radius": SCALED_R,
                      "scales": scales, "paths": sorted(set(paths)), "misplaced_per_layer": per_layer, "misplaced_scaled_stack": stacked,
                      "misplaced_unscaled_stack": unscaled}), flush=True)


def main():
    if "--demo" in sys.argv:
        return demo()
    R, reps = 15, int(arg("--reps", 3))
    label = arg("--label", "this tree")
    pairs = str(arg("--pairs", "u8,dn12")).split(",")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "stack_scaled_fused", "stack_scaled_fused_time_C2.jsonl"))
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    images = {"u8": lambda: (c.i0, c.i1), "dn12": lambda: (c.i0 * 16, c.i1 * 16)}
    d_xy, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray((c.n, 8), np.float32)
    R2 = api.stack_layer_radius(R, 2.0)
    with api.Context(0) as ctx:
        for pair in pairs:
            ctx.enable_timing(False)
            ctx.set_images(*images[pair]())
            ctx.stack_begin_wide(c.n, R, shift)
            d_lsh = DevArray(src=ctx.stack_layer_shift(2.0))
            search = ctx.match_ncc_wide_class_dev if pair == "u8" else ctx.match_ncc_wide_planes_dev
            configs = [(c.ocw, 1.0), (c.ocw, 2.0)] + ([(10, 2.0), (60, 2.0)] if pair == "u8" else [])
            for ocw, scale in configs:
                ctx.enable_timing(False)
                ctx.stack_begin_wide(c.n, R, shift)
                ctx.enable_timing(True)
                rl = api.stack_layer_radius(R, scale)
                calls = {"fused_scaled": lambda: ctx.stack_add_scaled_fused_dev(d_xy.ptr, c.n, c.offset, ocw, scale, 1.0, radius=rl)}
                if ocw == c.ocw and scale == 1.0:
                    calls["stack_add_fused"] = lambda: ctx.stack_add_fused_dev(d_xy.ptr, c.n, c.offset, ocw)
                elif ocw == c.ocw:
                    calls["stack_add_scaled"] = lambda: ctx.stack_add_scaled_dev(d_xy.ptr, c.n, c.offset, ocw, scale, 1.0, radius=rl)
                    calls["search"] = lambda: search(d_xy.ptr, c.n, c.offset, ocw, R2, 0, d_out.ptr, d_shift=d_lsh.ptr)
                ms, paths = {k: [] for k in calls}, {}
                for k in range(reps + 2):                                # one round = one call of each, interleaved
                    for name, call in calls.items():
                        call()
                        t = ctx.last_kernel_ms()
                        paths[name] = ctx.last_path()
                        if k >= 2:
                            ms[name].append(t)
                st = {k: stats(v) for k, v in ms.items()}
                rec = {"tree": label, "entry": "stack_scaled_fused", "pair": pair, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "scale": scale,
                       "layer_radius": rl, "reps": reps, "paths": paths, "ms": st, "all_ms": {k: [float(v) for v in ms[k]] for k in ms},
                       "state_bytes_per_layer": 20 * c.n * (2 * R + 1) ** 2, "layers": ctx.stack_info()[2]}
                if "stack_add_scaled" in st:
                    rec.update({"speedup": st["stack_add_scaled"]["median"] / st["fused_scaled"]["median"],
                                "every_fused_pass_faster_than_every_scaled_pass": bool(st["fused_scaled"]["max"] < st["stack_add_scaled"]["min"]),
                                "fused_minus_search_ms": st["fused_scaled"]["median"] - st["search"]["median"]})
                if "stack_add_fused" in st:
                    rec["scaled_minus_unscaled_ms"] = st["fused_scaled"]["median"] - st["stack_add_fused"]["median"]
                line = json.dumps(rec)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "a") as f:
                    f.write(line + "\n")
            ctx.enable_timing(False)
            ctx.stack_begin_wide(0, 0)                                   # (release the state before the next pair)
            d_lsh.free()


if __name__ == "__main__":
    main()
