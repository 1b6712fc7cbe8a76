#!/usr/bin/env python3
"""Time the exhaustive search on every pair the planes' matchers take (mimc3_match_ncc_full_dn) on BASELINE C2's pair and grid:
  python3 tools/full_dn_time.py [--reps K] [--label NAME] [--ocw 16,40] [--pairs dn16,u8,dn12]

One JSON line per run: the device time of a whole 200,000-point pass (HIP events through the context's timing hooks) -- median, mean,
min and max over K passes (default 20) after two warm-up passes:
  dn16    the pair as full-entropy 16-bit DN (256 * pixel + 8 random low bits, nulls kept) through the new entry, npeaks 0 and 4, with
          the share of points without / with nulls (host count);
  u8      the 8-bit pair through mimc3_match_ncc_full and through the new entry (the same kernels), npeaks 0;
  dn12    the pair times 16 (12-bit DN) through mimc3_match_ncc_full_planes and through the new entry (the same kernels), npeaks 0 and 4.
Run it twice in one session for the run-to-run spread.  Test / tuning infrastructure."""
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


def to_dn16(img, seed):
    low = np.random.default_rng(seed).integers(0, 256, img.shape).astype(np.float32)
    return np.ascontiguousarray(np.where(img == 0, np.float32(0), img * np.float32(256) + low).astype(np.float32))


def main():
    R, reps = 15, int(arg("--reps", 20))
    ocws = [int(v) for v in str(arg("--ocw", "16,40")).split(",") if v]
    pairs = str(arg("--pairs", "dn16,u8,dn12")).split(",")
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

        def dn(ocw, npk):
            return lambda: ctx.match_ncc_full_dn_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr if npk else 0, d_shift=d_sh.ptr)

        def planes(ocw, npk):
            return lambda: ctx.match_ncc_full_planes_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr if npk else 0,
                                                         d_shift=d_sh.ptr)

        for ocw in ocws:
            if "dn16" in pairs:
                i0, i1 = to_dn16(c.i0, 5), to_dn16(c.i1, 6)
                ctx.set_images(i0, i1)
                ds = dirty_share(i0, i1, c.xyuvav, c.offset, shift, ocw, R)
                for npk in (0, 4):
                    report("dn16", "match_ncc_full_dn", ocw, npk, dn(ocw, npk), dirty_share=ds)
            if "u8" in pairs:
                ctx.set_images(c.i0, c.i1)
                report("u8", "match_ncc_full", ocw, 0, lambda: ctx.match_ncc_full_dev(d_xy.ptr, c.n, c.offset, ocw, R, d_out.ptr, d_shift=d_sh.ptr))
                report("u8", "match_ncc_full_dn", ocw, 0, dn(ocw, 0))
            if "dn12" in pairs:
                ctx.set_images(c.i0 * 16, c.i1 * 16)
                for npk in (0, 4):
                    report("dn12", "match_ncc_full_planes", ocw, npk, planes(ocw, npk))
                    report("dn12", "match_ncc_full_dn", ocw, npk, dn(ocw, npk))


if __name__ == "__main__":
    main()
