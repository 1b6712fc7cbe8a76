#!/usr/bin/env python3
"""Time NCC stacking (mimc3_stack_*) on BASELINE C2's pair and grid, R 15, ocw 16:
  python3 tools/stack_time.py [--reps K] [--label NAME] [--ocw 16] [--out profiles/ncc_stack/stack_time_C2.jsonl]

One JSON line, printed and appended to --out: the device time (HIP events through the context's timing hooks), median, min and max over
K calls (default 10) after two warm-up calls, of
  search   match_ncc_full_any_dev(mode 1, npeaks 0, d_surf) alone: the float pass that writes every point's surface, in one launch;
  add      stack_add_dev: the same pass in chunks of STACK_CHUNK points into the layer scratch, each followed by stack_add_kernel
           (expected from the code: 24 bytes of traffic per cell on top of the pass, 4.6 GB at C2);
  finish   stack_finish_dev at npeaks 0 and 4, without the mean surface: 10 bytes per cell read.
Test / tuning infrastructure."""
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


def main():
    R, reps = 15, int(arg("--reps", 10))
    ocw = int(arg("--ocw", 16))
    label = arg("--label", "this tree")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "ncc_stack", "stack_time_C2.jsonl"))
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    NC = (2 * R + 1) ** 2
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        d_cand, d_surf = DevArray((4, c.n, 3), np.float32), DevArray((c.n, NC), np.float32)
        ctx.set_images(c.i0, c.i1)
        ctx.stack_begin(c.n, R, shift)
        ctx.enable_timing(True)

        def timed(call):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

        search = timed(lambda: ctx.match_ncc_full_any_dev(d_xy.ptr, c.n, c.offset, ocw, R, 0, d_out.ptr, d_shift=d_sh.ptr, mode=1,
                                                          d_surf=d_surf.ptr))
        add = timed(lambda: ctx.stack_add_dev(d_xy.ptr, c.n, c.offset, ocw))
        fin = {k: timed(lambda: ctx.stack_finish_dev(k, 1, d_out.ptr, d_cand=d_cand.ptr if k else 0)) for k in (0, 4)}
        layers = ctx.stack_info()[2]
        st = d_out.numpy()[:, 2]
        rec = {"tree": label, "entry": "stack", "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps, "layers": layers,
               "search_surf_ms": search, "stack_add_ms": add, "add_minus_search_ms": add["median"] - search["median"],
               "add_kernel_bytes": 24 * c.n * NC, "add_kernel_GBps": 24e-6 * c.n * NC / max(add["median"] - search["median"], 1e-9),
               "finish_k0_ms": fin[0], "finish_k4_ms": fin[4], "finish_bytes": 10 * c.n * NC,
               "finish_k0_GBps": 10e-6 * c.n * NC / fin[0]["median"], "stack_bytes": 10 * c.n * NC, "fit_share": float((st >= -1).mean())}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
