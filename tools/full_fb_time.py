#!/usr/bin/env python3
"""Time the forward-backward consistency check (mimc3_match_ncc_full_fb) on BASELINE C2's pair and grid:
  python3 tools/full_fb_time.py [--reps K] [--label NAME] [--ocw 16] [--pairs u8,dn16] [--npeaks 0,4]

One JSON line per (pair, ocw, npeaks): the device time (HIP events through the context's timing hooks) of
  single   one single-direction pass of mimc3_match_ncc_full_any with that npeaks -- the forward pass of the check;
  fb       the whole mimc3_match_ncc_full_fb_dev call: that pass, the seed kernel, the backward pass over (1 + npeaks) N rows (record only)
           and the compose kernel;
median, min and max over K calls (default 10) after two warm-up calls, R 15.  The expectation from the code is 1 + planes passes'
worth, planes = 1 + npeaks, plus two memory-bound elementwise kernels of under 100 bytes per row: "fb_over_single" is the measured
ratio, "searched" the share of the backward rows that are searched at all (the others leave their kernel at the header).
  u8     C2's 8-bit pair (the matrix-core kernels);  dn16  the pair as full-entropy 16-bit DN (the f32i kernels).
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
from full_planes_time import arg  # noqa: E402
from full_dn_time import to_dn16  # noqa: E402


def main():
    R, reps = 15, int(arg("--reps", 10))
    ocws = [int(v) for v in str(arg("--ocw", "16")).split(",") if v]
    pairs = str(arg("--pairs", "u8,dn16")).split(",")
    npks = [int(v) for v in str(arg("--npeaks", "0,4")).split(",") if v]
    label = arg("--label", "this tree")
    c = synth.make_case("C2")
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    kmax = max(npks)
    with api.Context(0) as ctx:
        d_xy, d_sh, d_out = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift), DevArray((c.n, 8), np.float32)
        d_cand = DevArray((max(kmax, 1), c.n, 3), np.float32)
        d_fb = DevArray((1 + kmax, c.n, 4), np.float32)
        ctx.enable_timing(True)

        def timed(call):
            ms = []
            for k in range(reps + 2):
                call()
                t = ctx.last_kernel_ms()
                if k >= 2:
                    ms.append(t)
            return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

        for pair in pairs:
            i0, i1 = (to_dn16(c.i0, 5), to_dn16(c.i1, 6)) if pair == "dn16" else (c.i0, c.i1)
            ctx.set_images(i0, i1)
            for ocw in ocws:
                for npk in npks:
                    single = timed(lambda: ctx.match_ncc_full_any_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_cand.ptr if npk else 0,
                                                                      d_shift=d_sh.ptr))
                    fb = timed(lambda: ctx.match_ncc_full_fb_dev(d_xy.ptr, c.n, c.offset, ocw, R, npk, d_out.ptr, d_fb.ptr,
                                                                 d_cand=d_cand.ptr if npk else 0, d_shift=d_sh.ptr))
                    st = d_fb.numpy()[:1 + npk, :, 2]
                    rec = {"tree": label, "pair": pair, "entry": "match_ncc_full_fb", "npeaks": npk, "planes": 1 + npk, "case": "C2", "n": c.n,
                           "ocw": ocw, "radius": R, "reps": reps, "path": ctx.last_path(), "single_ms": single, "fb_ms": fb,
                           "fb_over_single": fb["median"] / single["median"], "expected_passes": 2 + npk,
                           "searched": float(((st != -5) & (st != -6)).mean()),
                           "plane0_fit": float((st[0] >= -1).mean())}
                    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
