#!/usr/bin/env python3
"""Time the exhaustive search on an 8-bit pair at any chip size on the matrix cores (mimc3_match_ncc_full_chip_class) on BASELINE C2:
  python3 tools/full_chip_u8_time.py [--label NAME] [--out DIR]

C2's 8-bit pair, the points of tools/full_chip_time.py (C2's grid points whose chip and box at ocw 80, R 15 stay inside the image: about
189,000 of the 200,000), R 15, npeaks 0, one process, the configurations interleaved pass by pass, median of 3 passes after 2:
  (a) the new entry in mode 1 at ocw 7, 10, 11, 14, 16, 30, 40, 60, 80 (the matrix-core kernel, both forms);
  (b) match_ncc_full_chip_dev(mode 1) at the same ocw: the run-time-ocw float kernel, what such a call costs without the new kernel;
  (c) match_ncc_full_dev at 16 and 40: the templated matrix-core kernel, i.e. the price of a run-time ocw;
  (d) the clean form alone (MIMC3_CHIP_U8_FORMS=1), from which the masked form's share of (a) follows; the dirty share per ocw.
One JSON line per configuration with every pass, device time of a whole pass (HIP events through the context's timing hooks); `faster`
says whether EVERY pass of (a) was faster than EVERY pass of (b) -- the rule mode 0's dispatch follows.  With --out also written to
DIR/timings.jsonl.  Test / tuning infrastructure."""
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

OCWS = (7, 10, 11, 14, 16, 30, 40, 60, 80)


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
    configs = [(e, o) for o in OCWS for e in ("class", "class_clean_form", "full_chip")] + [("full", 16), ("full", 40)]
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=xy), DevArray(src=shift), DevArray((n, 8), np.float32)
        ctx.enable_timing(True)
        ctx.set_images(c.i0, c.i1)
        ms = {cfg: [] for cfg in configs}
        for k in range(warm + reps):
            for entry, ocw in configs:
                if entry == "full":
                    ctx.match_ncc_full_dev(d_xy.ptr, n, c.offset, ocw, R, d_out.ptr, d_shift=d_sh.ptr)
                    want = "u8_mfma_full"
                elif entry == "full_chip":
                    ctx.match_ncc_full_chip_dev(d_xy.ptr, n, c.offset, ocw, R, 0, d_out.ptr, 0, d_shift=d_sh.ptr, mode=1)
                    want = "f32g_chip"
                else:
                    if entry == "class_clean_form":
                        os.environ["MIMC3_CHIP_U8_FORMS"] = "1"
                    ctx.match_ncc_full_chip_class_dev(d_xy.ptr, n, c.offset, ocw, R, 0, d_out.ptr, 0, d_shift=d_sh.ptr, mode=1)
                    os.environ.pop("MIMC3_CHIP_U8_FORMS", None)
                    want = "u8_mfma_chip"
                t = ctx.last_kernel_ms()
                assert ctx.last_path() == want, (entry, ocw, ctx.last_path())
                if k >= warm:
                    ms[(entry, ocw)].append(t)
        lines = []
        for entry, ocw in configs:
            p = ms[(entry, ocw)]
            med = float(np.median(p))
            rec = {"tree": label, "pair": "8-bit", "entry": entry, "case": "C2", "n": n, "ocw": ocw, "radius": R, "reps": reps,
                   "pass_ms": [round(float(t), 4) for t in p], "pass_ms_median": med, "ns_per_point": 1e6 * med / n}
            if entry == "class":
                flt, cl = ms[("full_chip", ocw)], float(np.median(ms[("class_clean_form", ocw)]))
                rec["dirty_share"] = dirty_share(c.i0, c.i1, xy, c.offset, shift, ocw, R)
                rec["layout_kcw_ntr_kcv_lds"] = api.full_chip_class_layout(ocw)
                rec["clean_form_ms"], rec["masked_form_ms"] = cl, med - cl
                rec["float_kernel_over_this"] = float(np.median(flt)) / med
                rec["faster"] = bool(max(p) < min(flt))
                if ("full", ocw) in ms:
                    rec["ratio_to_templated_kernel"] = med / float(np.median(ms[("full", ocw)]))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, "timings.jsonl"), "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
