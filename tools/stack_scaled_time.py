#!/usr/bin/env python3
"""Time the scaled and weighted layers of NCC stacking (mimc3_stack_add_scaled) on BASELINE C2's pair and grid as floats, ocw 16, stack
R 15:
  python3 tools/stack_scaled_time.py [--reps K] [--label NAME] [--demo] [--out profiles/stack_scaled/stack_scaled_time_C2.jsonl]

One JSON line, printed and appended to --out: the device time (HIP events through the context's timing hooks), median, min and max over
K calls (default 3) after two warm-up calls, of
  add          stack_add_dev: the float pass at R 15 in chunks, each followed by stack_add_kernel (24 bytes of traffic per cell);
  scaled_s1    stack_add_scaled_dev at scale 1, weight 1, layer radius 15: the same pass and the same bytes through
               stack_add_scaled_kernel -- the gap to `add` is the new kernel's;
  search_r31   match_ncc_wide_dev(npeaks 0, d_surf) at R 31 alone, in one launch;
  scaled_s2    stack_add_scaled_dev at scale 2 (layer radius 31): that pass in chunks of stack_chunk(31) points, each followed by
               stack_add_scaled_kernel (4 bytes per layer cell read, 20 per stack cell read and written);
  finish       stack_finish_dev at npeaks 0 on the unweighted stack (10 bytes per cell), then -- after one add at weight 2 -- on the
               weighted one (18 bytes per cell).
--demo prints, on the device, the misplaced-point counts of tests/test_stack_scaled_cpu.py's series over six time baselines (per layer,
the scaled stack, the unscaled stack).
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
    from full_fb_common import FB_OFFSET
    from stack_common import misplaced
    from stack_scaled_common import SCALED_MOTION, SCALED_OCW, SCALED_R, layer_truth, scaled_series_pairs, scaled_series_points
    xy, shift = scaled_series_points()
    per_layer, scales = [], []
    with api.Context(0) as ctx, api.Context(0) as plain:
        ctx.stack_begin(xy.shape[0], SCALED_R, shift)
        plain.stack_begin(xy.shape[0], SCALED_R, shift)
        for s, i0, i1 in scaled_series_pairs():
            ctx.set_images(i0, i1)
            plain.set_images(i0, i1)
            rec = ctx.match_ncc_wide(xy, FB_OFFSET, SCALED_OCW, api.stack_layer_radius(SCALED_R, s), shift=ctx.stack_layer_shift(s))[0]
            per_layer.append(int(misplaced(rec, layer_truth(s)).sum()))
            scales.append(s)
            ctx.stack_add_scaled(xy, FB_OFFSET, SCALED_OCW, s)
            plain.stack_add(xy, FB_OFFSET, SCALED_OCW)
        stacked = int(misplaced(ctx.stack_finish()[0], SCALED_MOTION).sum())
        unscaled = int(misplaced(plain.stack_finish()[0], SCALED_MOTION).sum())
    print(json.dumps({"demo": "six time baselines", "n": int(xy.shape[0]), "ocw": SCALED_OCW, "radius": SCALED_R, "scales": scales,
                      "misplaced_per_layer": per_layer, "misplaced_scaled_stack": stacked, "misplaced_unscaled_stack": unscaled}), flush=True)


def main():
    if "--demo" in sys.argv:
        return demo()
    R, reps = 15, int(arg("--reps", 3))
    label = arg("--label", "this tree")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "stack_scaled", "stack_scaled_time_C2.jsonl"))
    c = synth.make_case("C2")
    ocw = c.ocw
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    f0, f1 = as_float(c.i0, 5), as_float(c.i1, 6)
    NC, R2 = (2 * R + 1) ** 2, api.stack_layer_radius(R, 2.0)
    d_xy, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray((c.n, 8), np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        ctx.match_ncc_wide(c.xyuvav[:8], c.offset, ocw, 16, shift=shift[:8])             # (the planes and the kernels' first load)
        ctx.stack_begin(c.n, R, shift)
        d_lsh = DevArray(src=ctx.stack_layer_shift(2.0))
        ctx.enable_timing(True)

        def timed(call):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

        add = timed(lambda: ctx.stack_add_dev(d_xy.ptr, c.n, c.offset, ocw))
        s1 = timed(lambda: ctx.stack_add_scaled_dev(d_xy.ptr, c.n, c.offset, ocw, 1.0, 1.0, radius=R))
        d_surf = DevArray((c.n, (2 * R2 + 1) ** 2), np.float32)
        search = timed(lambda: ctx.match_ncc_wide_dev(d_xy.ptr, c.n, c.offset, ocw, R2, 0, d_out.ptr, d_shift=d_lsh.ptr, d_surf=d_surf.ptr))
        d_surf.free()
        s2 = timed(lambda: ctx.stack_add_scaled_dev(d_xy.ptr, c.n, c.offset, ocw, 2.0, 1.0, radius=R2))
        fin = timed(lambda: ctx.stack_finish_dev(0, 1, d_out.ptr))
        assert not ctx.stack_weighted()
        ctx.stack_add_scaled_dev(d_xy.ptr, c.n, c.offset, ocw, 1.0, 2.0, radius=R)
        assert ctx.stack_weighted()
        finw = timed(lambda: ctx.stack_finish_dev(0, 1, d_out.ptr))
        st = d_out.numpy()[:, 2]
        rec = {"tree": label, "entry": "stack_scaled", "case": "C2 as floats", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
               "layers": ctx.stack_info()[2], "stack_add_ms": add, "scaled_s1_ms": s1, "s1_minus_add_ms": s1["median"] - add["median"],
               "layer_radius_s2": R2, "chunk_s2": min(api.stack_chunk(R), api.stack_chunk(R2)), "search_r31_surf_ms": search,
               "scaled_s2_ms": s2, "s2_minus_search_ms": s2["median"] - search["median"], "finish_ms": fin, "finish_weighted_ms": finw,
               "stack_bytes": 10 * c.n * NC, "stack_bytes_weighted": 18 * c.n * NC, "fit_share": float((st >= -1).mean())}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
