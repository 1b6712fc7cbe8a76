#!/usr/bin/env python3
"""Worked example: a velocity field from the exhaustive search's candidates and the post-matcher chain.

    python3 tools/full_multi_vmap.py [--ocw 15,16,30] [--npeaks 4] [--radius 7] [--seed 31]

On a synthetic 8-bit pair (synth.make_small: a known displacement, noise, null blobs) the exhaustive search with candidates
(Context.match_ncc_full_multi) runs once per chip size; the [npeaks][N][3] candidate blocks are stacked pass-major into
dp [ndp][N][3], ndp = len(ocw) * npeaks <= 64 -- the layout the DLC passes fill in mimc3_vmap -- and go through
Context.mimc2_postprocess (clustering, dpf0, dpf1, QM).  Prints one JSON line: how many grid points got a displacement, its median
and its worst error against the pair's true displacement, and the same for the single best peak (the record) for comparison.
A script, not library code: copy what you need."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mimc3_amd import api, synth  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    ocws = [int(v) for v in str(arg("--ocw", "15,16,30")).split(",")]
    npeaks, radius, seed = int(arg("--npeaks", 4)), int(arg("--radius", 7)), int(arg("--seed", 31))
    if len(ocws) * npeaks > 64:
        sys.exit("len(ocw) * npeaks must not exceed 64 (the post-matcher chain's ndp limit)")
    true = (3, -2)
    c = synth.make_small(seed=seed, shift=true, angle_deg=30.0, ocw=max(ocws), speed=900.0, h=300, w=320, dimx=12, dimy=10, noise_dn=3,
                         null_frac=0.03, margin=max(ocws) + 32)
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    mps = float(np.float32(c.xyuvav[1, 0] - c.xyuvav[0, 0]))
    with api.Context(0) as ctx:
        ctx.set_images(c.i0, c.i1)
        blocks, records = [], []
        for ocw in ocws:
            rec, cand = ctx.match_ncc_full_multi(c.xyuvav, c.offset, ocw, radius, npeaks, shift=shift)
            blocks.append(cand)
            records.append(rec)
        dp = np.concatenate(blocks)                                   # [ndp][N][3], pass-major
        field = ctx.mimc2_postprocess(dp, c.xyuvav, c.dimx, c.dimy, c.dt, c.mpp, mps).reshape(5, -1)
    du, dv = field[0] + c.offset[0], field[1] + c.offset[1]
    ok = ~np.isnan(du)
    rec = records[0]
    rok = rec[:, 2] >= -1
    print(json.dumps({
        "ocw": ocws, "npeaks": npeaks, "radius": radius, "ndp": int(dp.shape[0]), "points": int(c.n), "true": list(true),
        "chain": {"with_displacement": int(ok.sum()), "median": [float(np.median(du[ok])), float(np.median(dv[ok]))],
                  "worst_error_px": float(np.hypot(du[ok] - true[0], dv[ok] - true[1]).max())},
        "single_peak_ocw%d" % ocws[0]: {"with_peak": int(rok.sum()),
                                        "worst_error_px": float(np.hypot(rec[rok, 0] + c.offset[0] - true[0],
                                                                         rec[rok, 1] + c.offset[1] - true[1]).max())}}))


if __name__ == "__main__":
    main()
