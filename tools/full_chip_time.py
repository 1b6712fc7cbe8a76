#!/usr/bin/env python3
"""Time the exhaustive search at any chip size (mimc3_match_ncc_full_chip) on BASELINE C2's pair as floats:
  python3 tools/full_chip_time.py [--label NAME] [--out DIR]

C2's pair as floats (tools/full_any_time.py's), the points of C2's grid whose chip and box at ocw 80, R 15 stay inside the image
(about 189,000 of the 200,000), R 15, npeaks 0, one process, the configurations interleaved pass by pass, median of 3 passes after 2:
  (a) the price of a run-time ocw and of the bands: the new kernel in mode 1 at ocw 16 and 40 beside match_ncc_full_any_dev(mode 1);
  (b) the new ground: ocw 10, 20, 60 and 80, with the cost expected from the float kernel's ocw-16 pass scaled by CW^2.
One JSON line per configuration, device time of a whole pass (HIP events through the context's timing hooks); with --out also written
to DIR/timings.jsonl.  Test / tuning infrastructure."""
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
from full_planes_time import arg, dirty_share  # noqa: E402
from full_any_time import to_float  # noqa: E402


def main():
    R, reps, warm = 15, 3, 2
    label, out_dir = arg("--label", "this tree"), arg("--out", "")
    c = synth.make_case("C2")
    shift_all = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    H, W = c.i0.shape
    reach = api.full_chip_max_ocw() + R + 8
    u, v = c.xyuvav[:, 2], c.xyuvav[:, 3]
    keep = (u >= reach) & (u < W - reach) & (v >= reach) & (v < H - reach)
    xy, shift = np.ascontiguousarray(c.xyuvav[keep]), np.ascontiguousarray(shift_all[keep])
    n = xy.shape[0]
    i0, i1 = to_float(c.i0, 7), to_float(c.i1, 8)
    configs = [("full_any", 16), ("full_chip", 16), ("full_any", 40), ("full_chip", 40)] + [("full_chip", o) for o in (10, 20, 60, 80)]
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=xy), DevArray(src=shift), DevArray((n, 8), np.float32)
        ctx.enable_timing(True)
        ctx.set_images(i0, i1)
        ms = {cfg: [] for cfg in configs}
        for k in range(warm + reps):
            for entry, ocw in configs:
                call = ctx.match_ncc_full_any_dev if entry == "full_any" else ctx.match_ncc_full_chip_dev
                call(d_xy.ptr, n, c.offset, ocw, R, 0, d_out.ptr, 0, d_shift=d_sh.ptr, mode=1)
                t = ctx.last_kernel_ms()
                if k >= warm:
                    ms[(entry, ocw)].append(t)
        base = float(np.median(ms[("full_any", 16)]))
        lines = []
        for entry, ocw in configs:
            med = float(np.median(ms[(entry, ocw)]))
            rec = {"tree": label, "pair": "float", "entry": "match_ncc_" + entry, "mode": 1, "case": "C2", "n": n, "ocw": ocw, "radius": R,
                   "reps": reps, "band_rows": api.full_chip_band_rows(ocw, R), "pass_ms_median": med, "pass_ms_min": float(np.min(ms[(entry, ocw)])),
                   "pass_ms_max": float(np.max(ms[(entry, ocw)])), "ns_per_point": 1e6 * med / n,
                   "dirty_share": dirty_share(i0, i1, xy, c.offset, shift, ocw, R)}
            if entry == "full_chip":
                if ("full_any", ocw) in ms:
                    rec["ratio_to_full_any"] = med / float(np.median(ms[("full_any", ocw)]))
                expected = base * ((2 * ocw + 1) / 33.0) ** 2
                rec["expected_ms_cw2"] = expected
                rec["measured_over_expected"] = med / expected
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, "timings.jsonl"), "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
