#!/usr/bin/env python3
"""Time the exhaustive search beyond +-15 px (mimc3_match_ncc_wide) on BASELINE C2's pair and grid as floats, ocw 16:
  python3 tools/wide_time.py [--radii 15,16,23,31,47] [--npeaks 0,4] [--levels 2,3] [--reps K] [--tree LABEL] [--no-kres | --kres-only]

One JSON line per run: the device time of a whole 200,000-point pass (HIP events through the context's timing hooks) -- median, mean,
min and max over K passes (default 5) after two warm-up passes:
  match_ncc_wide          R 15 is the float kernel of match_ncc_full_any through the new entry (the yardstick of the same session);
                          R >= 16 the wide kernel.  `expected_ratio` is (2R + 1)^2 / 961, `ratio` the measured median over the R-15
                          median at the same npeaks;
  match_ncc_pyramid_any   R 15 at L levels, the other way to a range of (R + 1) 2^(L - 1) px, in the same session;
  kres                    tools/kres.py's VGPRs, SGPRs and scratch per instantiation (the compiler's view); LDS is sized at run time,
                          so the dynamic bytes per chip size and radius come from the library (mimc3_wide_lds_bytes).
Test / tuning infrastructure."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mimc3_amd import api, synth  # noqa: E402
from hipmem import DevArray  # noqa: E402
from pyramid_any_time import arg, as_float, timed  # noqa: E402


def kres_report(radii):
    """tools/kres.py on the two float search kernels, and -- LDS is dynamic there, so the compiler's report has none -- the bytes the
    library's own layout (mimc3_wide_lds_bytes) gives per chip size and radius."""
    for src in ("match_wide_kernel.hip", "match_full_f32g_kernel.hip"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), src], capture_output=True, text=True)
        for line in p.stdout.splitlines():
            print(json.dumps({"kres": src, "line": " ".join(line.split())}), flush=True)
    for ocw in (7, 15, 16, 30, 32, 40):
        rs = sorted({r for r in radii if 16 <= r <= api.wide_max_radius(ocw)} | {api.wide_max_radius(ocw)})
        print(json.dumps({"kernel": "match_ncc_wide", "ocw": ocw, "max_radius": api.wide_max_radius(ocw),
                          "dynamic_lds_bytes": {str(r): api.wide_lds_bytes(ocw, r) for r in rs}}), flush=True)


def main():
    radii = [int(v) for v in arg("--radii", "15,16,23,31,47").split(",")]
    npk = [int(v) for v in arg("--npeaks", "0,4").split(",")]
    levels = [int(v) for v in arg("--levels", "2,3").split(",") if v]
    reps = int(arg("--reps", "5"))
    tree = arg("--tree", "")
    if "--kres-only" in sys.argv:                           # (needs no GPU)
        return kres_report(radii)
    c = synth.make_case("C2")
    ocw = c.ocw
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    f0, f1 = as_float(c.i0, 5), as_float(c.i1, 6)
    base = {"tree": tree, "case": "C2 as floats", "n": c.n, "ocw": ocw, "reps": reps}
    d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
    d_out, d_so, d_cand = DevArray((c.n, 8), np.float32), DevArray((c.n, 2), np.int32), DevArray((8, c.n, 3), np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        ctx.match_ncc_wide(c.xyuvav[:8], c.offset, ocw, 15, shift=shift[:8])             # (the planes and the kernels' first load)
        ctx.enable_timing(True)
        yard = {}
        for R in radii:
            assert R <= api.wide_max_radius(ocw)
            for npeaks in npk:
                r = timed(ctx, reps, lambda: ctx.match_ncc_wide_dev(d_xy.ptr, c.n, c.offset, ocw, R, npeaks, d_out.ptr,
                                                                    d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr))
                if R == 15:
                    yard[npeaks] = r["pass_ms_median"]
                st = d_out.numpy()[:, 2]
                extra = {"expected_ratio": (2 * R + 1) ** 2 / 961.0}
                if npeaks in yard:
                    extra["ratio"] = r["pass_ms_median"] / yard[npeaks]
                if R >= 16:
                    extra["lds_bytes"] = api.wide_lds_bytes(ocw, R)
                print(json.dumps(dict(base, entry="match_ncc_wide", radius=R, npeaks=npeaks, path=ctx.last_path(), **r, **extra,
                                      ns_per_point=1e6 * r["pass_ms_median"] / c.n,
                                      status={"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()), "-3": int((st == -3).sum()),
                                              "-4": int((st == -4).sum())})), flush=True)
    for L in levels:
        with api.Context(0) as ctx:
            ctx.set_images(f0, f1)
            ctx.match_ncc_pyramid_any(c.xyuvav[:8], c.offset, ocw, 15, L, shift=shift[:8])
            ctx.enable_timing(True)
            for npeaks in npk:
                r = timed(ctx, reps, lambda: ctx.match_ncc_pyramid_any_dev(d_xy.ptr, c.n, c.offset, ocw, 15, L, npeaks, d_out.ptr,
                                                                           d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr, d_shift_out=d_so.ptr))
                print(json.dumps(dict(base, entry="match_ncc_pyramid_any", radius=15, levels=L, reach_px=16 * (1 << (L - 1)) - 1,
                                      npeaks=npeaks, path=ctx.last_path(), **r)), flush=True)
    if "--no-kres" not in sys.argv:
        kres_report(radii)


if __name__ == "__main__":
    main()
