#!/usr/bin/env python3
"""Time the coarse-to-fine exhaustive search on 12-bit and 16-bit pairs (mimc3_match_ncc_pyramid_dn) on BASELINE C2's pair and grid
(200,000 points, ocw 16, R 15, centred on the a-priori shift):
    python3 tools/pyramid_dn_time.py [--pairs dn12,dn16] [--levels 1,2,3] [--npeaks 0,4] [--reps K] [--tree LABEL] [--single-only]

dn12 is C2 times 16 plus 4 random low bits, dn16 is tests/full_dn_common.c2_dn16 (full low-order entropy); nulls stay null.  One JSON
line per (pair, levels, npeaks): the first call on a fresh context (host wall clock: the one-off build of the levels and their
tables, then the pass with its transfers), and the device time of a whole pass (HIP events through the context's timing hooks
around the _dev entry), median of K passes after 2 warm-ups.  Before them, per pair, the single-level entries the pyramid is
measured against (match_ncc_full_dn, and match_ncc_full_planes on dn12) -- --single-only stops there, which is what an older tree
without the pyramid entry can run.  Per-level kernel times come from a rocprofv3 --kernel-trace --stats run of this script.
Test / tuning infrastructure."""
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


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def dn12(img, seed):
    low = np.random.default_rng(seed).integers(0, 16, img.shape).astype(np.float32)
    return np.ascontiguousarray(np.where(img == 0, np.float32(0), img * np.float32(16) + low).astype(np.float32))


def dn16(img, seed):
    low = np.random.default_rng(seed).integers(0, 256, img.shape).astype(np.float32)
    return np.ascontiguousarray(np.where(img == 0, np.float32(0), img * np.float32(256) + low).astype(np.float32))


def timed(ctx, reps, call):
    ms = []
    for k in range(reps + 2):
        call()
        t = ctx.last_kernel_ms()
        if k >= 2:
            ms.append(t)
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_mean": float(np.mean(ms)), "pass_ms_min": float(np.min(ms)),
            "pass_ms_max": float(np.max(ms))}


def main():
    pairs = arg("--pairs", "dn12,dn16").split(",")
    levels = [int(v) for v in arg("--levels", "1,2,3").split(",")]
    npk = [int(v) for v in arg("--npeaks", "0,4").split(",")]
    reps = int(arg("--reps", "10"))
    tree = arg("--tree", "")
    c = synth.make_case("C2")
    ocw, R = c.ocw, 15
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    base = {"tree": tree, "case": "C2", "n": c.n, "ocw": ocw, "radius": R, "reps": reps}
    d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
    d_out, d_so, d_cand = DevArray((c.n, 8), np.float32), DevArray((c.n, 2), np.int32), DevArray((8, c.n, 3), np.float32)
    for pair in pairs:
        i0, i1 = (dn12(c.i0, 5), dn12(c.i1, 6)) if pair == "dn12" else (dn16(c.i0, 5), dn16(c.i1, 6))
        with api.Context(0) as ctx:
            ctx.set_images(i0, i1)
            ctx.match_ncc_full_dn(c.xyuvav[:8], c.offset, ocw, R, shift=shift[:8])       # (the level-0 planes, tables and the kernels' first load)
            ctx.enable_timing(True)
            entries = ["match_ncc_full_dn"] + (["match_ncc_full_planes"] if pair == "dn12" else [])
            for entry in entries:
                fn = getattr(ctx, entry + "_dev")
                for npeaks in npk:
                    r = timed(ctx, reps, lambda: fn(d_xy.ptr, c.n, c.offset, ocw, R, npeaks, d_out.ptr, d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr))
                    print(json.dumps(dict(base, pair=pair, entry=entry, npeaks=npeaks, path=ctx.last_path(), **r)), flush=True)
        if "--single-only" in sys.argv:
            continue
        for L in levels:
            with api.Context(0) as ctx:
                ctx.set_images(i0, i1)
                ctx.match_ncc_full_dn(c.xyuvav[:8], c.offset, ocw, R, shift=shift[:8])
                t0 = time.perf_counter()
                rec, _, _ = ctx.match_ncc_pyramid_dn(c.xyuvav, c.offset, ocw, R, L, shift=shift)
                first_ms = 1e3 * (time.perf_counter() - t0)
                ctx.enable_timing(True)
                for npeaks in npk:
                    r = timed(ctx, reps, lambda: ctx.match_ncc_pyramid_dn_dev(d_xy.ptr, c.n, c.offset, ocw, R, L, npeaks, d_out.ptr,
                                                                              d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr, d_shift_out=d_so.ptr))
                    out = d_out.numpy()
                    assert np.array_equal(out.view(np.uint32), rec.view(np.uint32))
                    st = out[:, 2]
                    print(json.dumps(dict(base, pair=pair, entry="match_ncc_pyramid_dn", levels=L, npeaks=npeaks, path=ctx.last_path(),
                                          first_call_ms_wall=first_ms, **r,
                                          status={"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()), "-3": int((st == -3).sum()),
                                                  "-4": int((st == -4).sum()), "nan": int(np.isnan(st).sum())})), flush=True)


if __name__ == "__main__":
    main()
