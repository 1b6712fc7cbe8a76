#!/usr/bin/env python3
"""Time the exhaustive search on any f32 pair (mimc3_match_ncc_full_any) on BASELINE C2's pair and grid:
  python3 tools/full_any_time.py [--reps K] [--label NAME] [--ocw 16,40] [--pairs float,float_clean,dn16,dn16_clean]

One JSON line per run: the device time of a whole 200,000-point pass (HIP events through the context's timing hooks) -- median, mean,
min and max over K passes (default 10) after two warm-up passes, npeaks 0 and 4, R 15:
  float        C2's pair as floats, pixel * 0.37 + U(0, 0.37) where non-null (f32), nulls kept: the float kernel (mode 0), with the share
               of points that have an excluded pixel in the chip or the box (host count: they run the dirty body);
  float_clean  the same pair with every null filled with a float in (0, 0.37]: only the points whose box leaves the image stay dirty;
  dn16         the pair as full-entropy 16-bit DN through mimc3_match_ncc_full_dn (the f32i kernels), the figures beside which
               DESIGN 4.1h reads the float kernel's;
  dn16_clean   the same with every null filled (DN 256 + low bits): the f32i clean kernel alone, but for the boxes that leave the image.
The ns per clean and per dirty point of DESIGN 4.1h solve each class's two lines for its two bodies:
  t = (1 - dirty_share) * clean + dirty_share * dirty.
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
from full_planes_time import arg, dirty_share  # noqa: E402
from full_dn_time import to_dn16  # noqa: E402


def to_float(img, seed, fill_nulls=False):
    u = np.random.default_rng(seed).random(img.shape).astype(np.float32) * np.float32(0.37)
    f = (img * np.float32(0.37) + u).astype(np.float32)
    if fill_nulls:
        return np.ascontiguousarray(np.maximum(f, np.float32(1e-3)))
    return np.ascontiguousarray(np.where(img == 0, np.float32(0), f).astype(np.float32))


def main():
    R, reps = 15, int(arg("--reps", 10))
    ocws = [int(v) for v in str(arg("--ocw", "16,40")).split(",") if v]
    pairs = str(arg("--pairs", "float,float_clean,dn16,dn16_clean")).split(",")
    label = arg("--label", "this tree")
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        d_cand = DevArray((4, c.n, 3), np.float32)
        ctx.enable_timing(True)

        def report(pair, entry, ocw, npk, call, **extra):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            rec = {"tree": label, "pair": pair, "entry": entry, "npeaks": npk, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps,
                   "path": ctx.last_path(), "pass_ms_median": float(np.median(ms)), "pass_ms_mean": float(np.mean(ms)),
                   "pass_ms_min": float(np.min(ms)), "pass_ms_max": float(np.max(ms)), "ns_per_point": 1e6 * float(np.median(ms)) / c.n}
            rec.update(extra)
            print(json.dumps(rec), flush=True)

        def anyp(ocw, npk):
            return lambda: ctx.match_ncc_full_any_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr if npk else 0, d_shift=d_sh.ptr)

        def dn(ocw, npk):
            return lambda: ctx.match_ncc_full_dn_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr if npk else 0, d_shift=d_sh.ptr)

        for pair in pairs:
            if pair == "dn16":
                i0, i1 = to_dn16(c.i0, 5), to_dn16(c.i1, 6)
            elif pair == "dn16_clean":
                i0, i1 = to_dn16(np.maximum(c.i0, 1), 5), to_dn16(np.maximum(c.i1, 1), 6)
            else:
                i0, i1 = to_float(c.i0, 7, pair == "float_clean"), to_float(c.i1, 8, pair == "float_clean")
            ctx.set_images(i0, i1)
            for ocw in ocws:
                ds = dirty_share(i0, i1, c.xyuvav, c.offset, shift, ocw, R)
                for npk in (0, 4):
                    if pair.startswith("dn16"):
                        report(pair, "match_ncc_full_dn", ocw, npk, dn(ocw, npk), dirty_share=ds)
                    else:
                        report(pair, "match_ncc_full_any", ocw, npk, anyp(ocw, npk), dirty_share=ds)


if __name__ == "__main__":
    main()
