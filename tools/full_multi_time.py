#!/usr/bin/env python3
"""Time the exhaustive search with candidates (mimc3_match_ncc_full_multi) on BASELINE C2's pair and grid, next to the single-peak
entry on the same tree:  python3 tools/full_multi_time.py [--radius R] [--reps K] [--npeaks 1,2,4,8] [--label NAME]

One JSON line per entry and npeaks: the device time of a whole 200,000-point pass (HIP events through the context's timing hooks: the
flag reset and the three form launches) -- median, mean, min and max over K passes (default 20) after two warm-up passes.  A tree
without the candidates entry (the parent commit) gives the single-peak line alone: run it there in the same session for the baseline
and its run-to-run spread.  The per-form kernel times come from a rocprofv3 --kernel-trace --stats run of this script; the tail's
cycles from MIMC3_MX_STATS=1 (phase 5 of a candidates kernel is the record's tail, phase 6 the candidates' tail).  Test / tuning
infrastructure."""
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


def main():
    R, reps = int(arg("--radius", 15)), int(arg("--reps", 20))
    peaks = [int(v) for v in str(arg("--npeaks", "1,2,4,8")).split(",") if v]
    label = arg("--label", "this tree")
    c = synth.make_case("C2")
    ocw = c.ocw
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    multi = hasattr(api.Context, "match_ncc_full_multi_dev")
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        d_cand = DevArray((8, c.n, 3), np.float32) if multi else None
        ctx.enable_timing(True)

        def timed(call):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            return ms

        runs = [("match_ncc_full", 0, lambda: ctx.match_ncc_full_dev(d_xy.ptr, c.n, c.offset, ocw, R, d_out.ptr, d_shift=d_sh.ptr))]
        if multi:
            for npk in peaks:
                runs.append(("match_ncc_full_multi", npk, lambda npk=npk: ctx.match_ncc_full_multi_dev(
                    d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr, d_shift=d_sh.ptr)))
        for entry, npk, call in runs:
            ms = timed(call)
            rec = {"tree": label, "entry": entry, "npeaks": npk, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                   "pass_ms_median": float(np.median(ms)), "pass_ms_mean": float(np.mean(ms)), "pass_ms_min": float(np.min(ms)),
                   "pass_ms_max": float(np.max(ms)), "ns_per_point": 1e6 * float(np.median(ms)) / c.n}
            if npk:
                cd = d_cand.numpy()[:npk]
                rec["slots_filled"] = float((cd[:, :, 2] >= -1).mean())
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
