#!/usr/bin/env python3
"""Time NCC stacking and forward-backward consistency beyond +-15 px (mimc3_stack_begin_wide, mimc3_match_ncc_wide_fb) on BASELINE C2's
pair and grid as floats, ocw 16:
  python3 tools/wide_stack_time.py [--radii 16,31,47] [--reps K] [--label NAME] [--no-fb] [--demo]
                                   [--out profiles/full_search_wide_stack/wide_stack_time_C2.jsonl]

One JSON line per radius, printed and appended to --out: the device time (HIP events through the context's timing hooks), median, min
and max over K calls (default 3) after two warm-up calls, of
  search   match_ncc_wide_dev(npeaks 0, d_surf) alone: the wide pass that writes every point's surface, in one launch;
  add      stack_add_dev: the same pass in chunks of stack_chunk(R) points into the layer scratch, each followed by stack_add_kernel
           (expected from the code: the pass plus 24 bytes of traffic per cell);
  finish   stack_finish_dev at npeaks 0 and 4, without the mean surface: stack_tail_wide_kernel, 10 bytes per cell read;
  fb       match_ncc_wide_fb_dev at npeaks 0 and 4 beside one match_ncc_wide_dev pass at the same npeaks (expected from the code:
           1 + (1 + npeaks) wide passes plus two elementwise kernels);
and the size of the stack's state (10 bytes per cell: 18 GB at 200,000 points and R 47).
--demo prints, on the device, the misplaced-point counts of tests/test_wide_stack_cpu.py's series (per layer and stacked).
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
from pyramid_any_time import arg, as_float  # noqa: E402


def demo():
    from stack_common import misplaced
    from test_wide_stack_cpu import FAR_STACK_OCW, FAR_STACK_R, far_series
    from wide_common import FAR_TRUE
    series = far_series()
    per_layer = []
    with api.Context(0) as ctx:
        ctx.stack_begin_wide(series[0].n, FAR_STACK_R)
        for c in series:
            ctx.set_images(c.i0, c.i1)
            per_layer.append(int(misplaced(ctx.match_ncc_wide(c.xyuvav, (0, 0), FAR_STACK_OCW, FAR_STACK_R)[0], FAR_TRUE).sum()))
            ctx.stack_add(c.xyuvav, (0, 0), FAR_STACK_OCW)
        stacked = int(misplaced(ctx.stack_finish()[0], FAR_TRUE).sum())
    print(json.dumps({"demo": "far series", "n": series[0].n, "ocw": FAR_STACK_OCW, "radius": FAR_STACK_R, "misplaced_per_layer": per_layer,
                      "misplaced_stacked": stacked}), flush=True)


def main():
    if "--demo" in sys.argv:
        return demo()
    radii = [int(v) for v in arg("--radii", "16,31,47").split(",")]
    reps = int(arg("--reps", 3))
    label = arg("--label", "this tree")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "full_search_wide_stack", "wide_stack_time_C2.jsonl"))
    c = synth.make_case("C2")
    ocw = c.ocw
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    f0, f1 = as_float(c.i0, 5), as_float(c.i1, 6)
    d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
    d_cand, d_fb = DevArray((4, c.n, 3), np.float32), DevArray((5, c.n, 4), np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        ctx.match_ncc_wide(c.xyuvav[:8], c.offset, ocw, 16, shift=shift[:8])             # (the planes and the kernel's first load)

        def timed(call):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

        for R in radii:
            assert 16 <= R <= api.wide_max_radius(ocw)
            NC = (2 * R + 1) ** 2
            ctx.enable_timing(False)
            ctx.stack_begin_wide(c.n, R, shift)
            d_surf = DevArray((c.n, NC), np.float32)
            ctx.enable_timing(True)
            search = timed(lambda: ctx.match_ncc_wide_dev(d_xy.ptr, c.n, c.offset, ocw, R, 0, d_out.ptr, d_shift=d_sh.ptr, d_surf=d_surf.ptr))
            d_surf.free()                                                                # (7.2 GB at R 47)
            add = timed(lambda: ctx.stack_add_dev(d_xy.ptr, c.n, c.offset, ocw))
            fin = {k: timed(lambda: ctx.stack_finish_dev(k, 1, d_out.ptr, d_cand=d_cand.ptr if k else 0)) for k in (0, 4)}
            layers = ctx.stack_info()[2]
            st = d_out.numpy()[:, 2]
            rec = {"tree": label, "entry": "stack_wide", "case": "C2 as floats", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                   "layers": layers, "chunk": api.stack_chunk(R), "search_surf_ms": search, "stack_add_ms": add,
                   "add_minus_search_ms": add["median"] - search["median"], "add_kernel_bytes": 24 * c.n * NC,
                   "add_kernel_GBps": 24e-6 * c.n * NC / max(add["median"] - search["median"], 1e-9),
                   "finish_k0_ms": fin[0], "finish_k4_ms": fin[4], "finish_bytes": 10 * c.n * NC,
                   "finish_k0_GBps": 10e-6 * c.n * NC / fin[0]["median"], "stack_bytes": 10 * c.n * NC, "fit_share": float((st >= -1).mean())}
            if "--no-fb" not in sys.argv:
                for k in (0, 4):
                    one = timed(lambda: ctx.match_ncc_wide_dev(d_xy.ptr, c.n, c.offset, ocw, R, k, d_out.ptr, d_cand.ptr if k else 0,
                                                               d_shift=d_sh.ptr))
                    fb = timed(lambda: ctx.match_ncc_wide_fb_dev(d_xy.ptr, c.n, c.offset, ocw, R, k, d_out.ptr, d_fb.ptr,
                                                                 d_cand=d_cand.ptr if k else 0, d_shift=d_sh.ptr))
                    err = d_fb.numpy()[0, :, 3]
                    rec.update({f"wide_k{k}_ms": one, f"wide_fb_k{k}_ms": fb, f"fb_k{k}_passes": fb["median"] / one["median"],
                                f"fb_k{k}_expected_passes": 2 + k, f"fb_k{k}_err_below_quarter_px": float((err < 0.25).mean())})
            ctx.enable_timing(False)
            ctx.stack_begin_wide(0, 0)                                                   # (release the state before the next radius)
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
