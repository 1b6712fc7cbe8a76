#!/usr/bin/env python3
"""Time the coarse-to-fine exhaustive search (mimc3_match_ncc_pyramid) on BASELINE C2's pair and grid (ocw 16, R 15, centred on the
a-priori shift):  python3 tools/pyramid_time.py [--levels 1,2,3,4] [--reps K]

One JSON line per level count: the first call on a fresh context (host wall clock: the one-off build of the pyramid levels and
their tables, then the pass with its transfers), the device time of a whole pass over K passes after it (HIP events through the
context's timing hooks around the _dev entry: the steps between the levels, every level's flag reset and form launches) and the
statuses.  Per-level kernel times come from a rocprofv3 --kernel-trace --stats run of this script (each level's forms are separate
kernel launches; the level-l planes are 4^l times smaller, the surfaces cost the same).  Test / tuning infrastructure."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mimc3_amd import api, synth  # noqa: E402
from hipmem import DevArray  # noqa: E402


def main():
    levels = [int(v) for v in sys.argv[sys.argv.index("--levels") + 1].split(",")] if "--levels" in sys.argv else [1, 2, 3, 4]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    c = synth.make_case("C2")
    ocw, R = c.ocw, 15
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    for L in levels:
        with api.Context(0) as ctx:
            ctx.set_images(c.i0, c.i1)
            ctx.match_ncc_full(c.xyuvav[:8], c.offset, ocw, R, shift=shift[:8])       # (the level-0 tables and the kernels' first load)
            t0 = time.perf_counter()
            rec, _ = ctx.match_ncc_pyramid(c.xyuvav, c.offset, ocw, R, L, shift=shift)
            first_ms = 1e3 * (time.perf_counter() - t0)
            d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
            d_out, d_so = DevArray((c.n, 8), np.float32), DevArray((c.n, 2), np.int32)
            ctx.enable_timing(True)
            ms = []
            for k in range(reps + 2):
                ctx.match_ncc_pyramid_dev(d_xy.ptr, c.n, c.offset, ocw, R, L, d_out.ptr, d_shift=d_sh.ptr, d_shift_out=d_so.ptr)
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            out = d_out.numpy()
        assert np.array_equal(out.view(np.uint32), rec.view(np.uint32))
        st = out[:, 2]
        print(json.dumps({"case": "C2", "n": c.n, "ocw": ocw, "radius": R, "levels": L, "reps": reps,
                          "first_call_ms_wall": first_ms, "pass_ms_mean": float(np.mean(ms)), "pass_ms_median": float(np.median(ms)),
                          "pass_ms_min": float(np.min(ms)), "status": {"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()),
                                                                        "-3": int((st == -3).sum()), "-4": int((st == -4).sum()),
                                                                        "nan": int(np.isnan(st).sum())}}), flush=True)


if __name__ == "__main__":
    main()
