#!/usr/bin/env python3
"""Time the exhaustive search (mimc3_match_ncc_full) on BASELINE C2's pair and grid:  python3 tools/full_search_time.py [--radius R] [--reps K]

One JSON line: the device time of a whole 200,000-point pass (HIP events through the context's timing hooks: the flag reset and the
three form launches), the mean over K passes after a warm-up, and how many points each form takes (clean / window nulls only /
general), classified on the host from the null counts of each chip and search box.  The per-form kernel times come from a
rocprofv3 --kernel-trace --stats run of this script (the three forms are separate kernels).  Test / tuning infrastructure."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mimc3_amd import api, synth  # noqa: E402
from hipmem import DevArray  # noqa: E402


def box_nulls(img, us, vs, half):
    """null pixels of the (2 half + 1)^2 boxes centred at (us, vs); pixels outside the image count as nulls"""
    H, W = img.shape
    pad = half + 1
    z = np.pad((img == 0).astype(np.int64), pad, constant_values=1)
    sat = np.zeros((z.shape[0] + 1, z.shape[1] + 1), np.int64)
    sat[1:, 1:] = z.cumsum(0).cumsum(1)
    u0, v0 = us - half + pad, vs - half + pad
    u1, v1 = u0 + 2 * half + 1, v0 + 2 * half + 1
    return sat[v1, u1] - sat[v0, u1] - sat[v1, u0] + sat[v0, u0]


def main():
    R = int(sys.argv[sys.argv.index("--radius") + 1]) if "--radius" in sys.argv else 15
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    c = synth.make_case("C2")
    ocw = c.ocw
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    u0, v0 = c.xyuvav[:, 2].astype(np.int64), c.xyuvav[:, 3].astype(np.int64)
    chip_n = box_nulls(c.i0, u0, v0, ocw)
    box_n = box_nulls(c.i1, u0 + c.offset[0] + shift[:, 0], v0 + c.offset[1] + shift[:, 1], R + ocw)
    forms = {"clean": int(((chip_n == 0) & (box_n == 0)).sum()), "window_nulls": int(((chip_n == 0) & (box_n > 0)).sum()),
             "general": int((chip_n > 0).sum())}
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        ctx.enable_timing(True)
        ms = []
        for k in range(reps + 2):
            ctx.match_ncc_full_dev(d_xy.ptr, c.n, c.offset, ocw, R, d_out.ptr, d_shift=d_sh.ptr)
            t = ctx.last_kernel_ms()
            if k >= 2:
                ms.append(t)
        out = d_out.numpy()
    st = out[:, 2]
    print(json.dumps({"case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps, "pass_ms_mean": float(np.mean(ms)),
                      "pass_ms_median": float(np.median(ms)), "pass_ms_min": float(np.min(ms)), "ns_per_point": 1e6 * float(np.median(ms)) / c.n,
                      "points_per_form": forms, "status": {"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()),
                                                           "-3": int((st == -3).sum()), "-4": int((st == -4).sum())}}))


if __name__ == "__main__":
    main()
