#!/usr/bin/env python3
"""Time stack layers through the class kernels (mimc3_stack_add_class) on BASELINE C2's pair and grid, R 15, ocw 16:
  python3 tools/stack_class_time.py [--reps 3] [--label NAME] [--ocw 16] [--pairs u8,dn12,dn16] [--out profiles/stack_class/stack_class_time_C2.jsonl]
  python3 tools/stack_class_time.py --full-only [--reps 10] [--label NAME] [--out ...]

One JSON line per pair, printed and appended to --out.  C2 as 8-bit, as 12-bit DN (times 16) and as full-entropy 16-bit DN, in ONE
process; per pair the four calls are interleaved -- one round is one call of each -- and the device time of every call (HIP events
through the context's timing hooks) is kept: median, min and max over K rounds (default 3) after two warm-up rounds, of
  stack_add        stack_add_dev: every layer through the float kernel;
  stack_add_class  stack_add_class_dev: the layer through the kernel of the pair's class;
  search_surf      match_ncc_full_surf_dev alone (npeaks 0): the class kernel's search with the surface store;
  search           match_ncc_full_dn_dev alone (npeaks 0): the class kernel's search without surfaces.
Derived: surf_store_ms = search_surf - search (medians), speedup = stack_add / stack_add_class, and whether the class layer is faster
than stack_add by more than the spread (max - min) of either.

--full-only times match_ncc_full_dev on the 8-bit pair alone (one JSON line): the entry that existed before, for an A/B of two builds
-- run it alternately with MIMC3_TREE pointing at a checkout of the parent commit and at this one.  Test / tuning infrastructure."""
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
from full_dn_time import to_dn16  # noqa: E402

R = 15


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def emit(rec, out_path):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def main():
    full_only = "--full-only" in sys.argv
    reps = int(arg("--reps", 10 if full_only else 3))
    ocw = int(arg("--ocw", 16))
    pairs = str(arg("--pairs", "u8,dn12,dn16")).split(",")
    label = arg("--label", "this tree")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "stack_class", "stack_class_time_C2.jsonl"))
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    NC = (2 * R + 1) ** 2
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        ctx.enable_timing(True)
        if full_only:
            ctx.set_images(c.i0, c.i1)
            ms = []
            for k in range(reps + 2):
                ctx.match_ncc_full_dev(d_xy.ptr, c.n, c.offset, ocw, R, d_out.ptr, d_shift=d_sh.ptr)
                if k >= 2:
                    ms.append(ctx.last_kernel_ms())
            emit({"tree": label, "entry": "match_ncc_full", "pair": "u8", "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                  "path": ctx.last_path(), "pass_ms": stats(ms), "all_ms": [float(v) for v in ms]}, out_path)
            return
        d_surf = DevArray((c.n, NC), np.float32)
        ctx.stack_begin(c.n, R, shift)
        images = {"u8": lambda: (c.i0, c.i1), "dn12": lambda: (c.i0 * 16, c.i1 * 16), "dn16": lambda: (to_dn16(c.i0, 5), to_dn16(c.i1, 6))}
        calls = {
            "stack_add": lambda: ctx.stack_add_dev(d_xy.ptr, c.n, c.offset, ocw),
            "stack_add_class": lambda: ctx.stack_add_class_dev(d_xy.ptr, c.n, c.offset, ocw),
            "search_surf": lambda: ctx.match_ncc_full_surf_dev(d_xy.ptr, c.n, c.offset, ocw, R, 0, d_out.ptr, d_surf.ptr, d_shift=d_sh.ptr),
            "search": lambda: ctx.match_ncc_full_dn_dev(d_xy.ptr, c.n, c.offset, ocw, R, 0, d_out.ptr, d_shift=d_sh.ptr),
        }
        for pair in pairs:
            ctx.set_images(*images[pair]())
            ms, paths = {k: [] for k in calls}, {}
            for k in range(reps + 2):                                # one round = one call of each, interleaved
                for name, call in calls.items():
                    call()
                    t = ctx.last_kernel_ms()
                    paths[name] = ctx.last_path()
                    if k >= 2:
                        ms[name].append(t)
            st = {k: stats(v) for k, v in ms.items()}
            spread = {k: st[k]["max"] - st[k]["min"] for k in st}
            gain = st["stack_add"]["median"] - st["stack_add_class"]["median"]
            emit({"tree": label, "entry": "stack_class", "pair": pair, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                  "paths": paths, "stack_add_ms": st["stack_add"], "stack_add_class_ms": st["stack_add_class"],
                  "search_surf_ms": st["search_surf"], "search_ms": st["search"],
                  "surf_store_ms": st["search_surf"]["median"] - st["search"]["median"], "surf_bytes": 4 * c.n * NC,
                  "accumulate_ms": st["stack_add_class"]["median"] - st["search_surf"]["median"],
                  "speedup": st["stack_add"]["median"] / st["stack_add_class"]["median"], "gain_ms": gain,
                  "spread_ms": spread, "faster_by_more_than_spread": bool(gain > max(spread["stack_add"], spread["stack_add_class"])),
                  "layers": ctx.stack_info()[2]}, out_path)


if __name__ == "__main__":
    main()
