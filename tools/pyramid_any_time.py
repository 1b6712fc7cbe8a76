#!/usr/bin/env python3
"""Time the coarse-to-fine exhaustive search on a float pair (mimc3_match_ncc_pyramid_any) on BASELINE C2's pair and grid as floats
(pixel * 0.37 + U(0, 0.37), nulls kept; 200,000 points, ocw 16, R 15, centred on the a-priori shift):
    python3 tools/pyramid_any_time.py [--levels 1,2,3] [--npeaks 0,4] [--reps K] [--tree LABEL] [--single-only] [--no-dirty]

One JSON line per (levels, npeaks): the first call on a fresh context (host wall clock: the one-off build of the float levels, then the
pass with its transfers), and the device time of a whole pass (HIP events through the context's timing hooks around the _dev entry),
median of K passes after 2 warm-ups.  Before them the single-level entry the pyramid is measured against (match_ncc_full_any) --
--single-only stops there, which is what an older tree without the pyramid entry can run -- and, counted on the CPU, the share of the
points whose chip or search box holds an excluded pixel on every level (the float kernel's masked body takes those; the box is placed
at the a-priori displacement scaled to the level).  Per-level kernel times come from a rocprofv3 --kernel-trace --stats run of this
script.  Test / tuning infrastructure."""
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


def as_float(img, seed):
    u = np.random.default_rng(seed).random(img.shape).astype(np.float32) * np.float32(0.37)
    return np.ascontiguousarray(np.where(img == 0, np.float32(0), img * np.float32(0.37) + u).astype(np.float32))


def timed(ctx, reps, call):
    ms = []
    for k in range(reps + 2):
        call()
        t = ctx.last_kernel_ms()
        if k >= 2:
            ms.append(t)
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_mean": float(np.mean(ms)), "pass_ms_min": float(np.min(ms)),
            "pass_ms_max": float(np.max(ms))}


def dirty_shares(f0, f1, xy, D, ocw, R, levels):
    """Per level 0 .. levels - 1: the share of the points with an excluded pixel (< 1e-10 or NaN) in the chip or in the search box."""
    from pyramid_any_oracle import reduce2_any
    uv0 = xy[:, 2:4].astype(np.int64)
    out = []
    for lv in range(levels):
        if lv:
            f0, f1 = reduce2_any(f0), reduce2_any(f1)
        H, W = f0.shape
        pad = 256
        tabs = []
        for f in (f0, f1):
            ex = np.ones((H + 2 * pad, W + 2 * pad), np.int64)                     # (the zero border is excluded too)
            ex[pad:pad + H, pad:pad + W] = ~(f.astype(np.float64) >= 1e-10)
            t = np.zeros((H + 2 * pad + 1, W + 2 * pad + 1), np.int64)
            t[1:, 1:] = ex.cumsum(0).cumsum(1)
            tabs.append(t)

        def count(t, cu, cv, h):
            x0, x1 = np.clip(cu - h + pad, 0, W + 2 * pad), np.clip(cu + h + 1 + pad, 0, W + 2 * pad)
            y0, y1 = np.clip(cv - h + pad, 0, H + 2 * pad), np.clip(cv + h + 1 + pad, 0, H + 2 * pad)
            return t[y1, x1] - t[y0, x1] - t[y1, x0] + t[y0, x0]
        pos = uv0 >> lv
        d = D if lv == 0 else (D + (1 << (lv - 1))) >> lv
        inside = (pos[:, 0] - ocw >= 0) & (pos[:, 0] + ocw < W) & (pos[:, 1] - ocw >= 0) & (pos[:, 1] + ocw < H)
        dirty = (count(tabs[0], pos[:, 0], pos[:, 1], ocw) > 0) | (count(tabs[1], pos[:, 0] + d[:, 0], pos[:, 1] + d[:, 1], ocw + R) > 0)
        out.append({"level": lv, "searched": int(inside.sum()), "dirty_share": float(dirty[inside].mean()) if inside.any() else 0.0})
    return out


def main():
    levels = [int(v) for v in arg("--levels", "1,2,3").split(",")]
    npk = [int(v) for v in arg("--npeaks", "0,4").split(",")]
    reps = int(arg("--reps", "10"))
    tree = arg("--tree", "")
    c = synth.make_case("C2")
    ocw, R = c.ocw, 15
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    f0, f1 = as_float(c.i0, 5), as_float(c.i1, 6)
    base = {"tree": tree, "case": "C2 as floats", "n": c.n, "ocw": ocw, "radius": R, "reps": reps}
    d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
    d_out, d_so, d_cand = DevArray((c.n, 8), np.float32), DevArray((c.n, 2), np.int32), DevArray((8, c.n, 3), np.float32)
    with api.Context(0) as ctx:
        ctx.set_images(f0, f1)
        ctx.match_ncc_full_any(c.xyuvav[:8], c.offset, ocw, R, shift=shift[:8])          # (the level-0 planes and the kernels' first load)
        ctx.enable_timing(True)
        for npeaks in npk:
            r = timed(ctx, reps, lambda: ctx.match_ncc_full_any_dev(d_xy.ptr, c.n, c.offset, ocw, R, npeaks, d_out.ptr,
                                                                    d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr))
            print(json.dumps(dict(base, entry="match_ncc_full_any", npeaks=npeaks, path=ctx.last_path(), **r)), flush=True)
    if "--single-only" in sys.argv:
        return
    if "--no-dirty" not in sys.argv:
        D = np.asarray(c.offset, np.int64).reshape(1, 2) + shift.astype(np.int64)
        print(json.dumps(dict(base, dirty=dirty_shares(f0, f1, c.xyuvav, D, ocw, R, max(levels)))), flush=True)
    for L in levels:
        with api.Context(0) as ctx:
            ctx.set_images(f0, f1)
            ctx.match_ncc_full_any(c.xyuvav[:8], c.offset, ocw, R, shift=shift[:8])
            t0 = time.perf_counter()
            rec, _, _ = ctx.match_ncc_pyramid_any(c.xyuvav, c.offset, ocw, R, L, shift=shift)
            first_ms = 1e3 * (time.perf_counter() - t0)
            ctx.enable_timing(True)
            for npeaks in npk:
                r = timed(ctx, reps, lambda: ctx.match_ncc_pyramid_any_dev(d_xy.ptr, c.n, c.offset, ocw, R, L, npeaks, d_out.ptr,
                                                                           d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr, d_shift_out=d_so.ptr))
                out = d_out.numpy()
                if npeaks == 0:
                    assert np.array_equal(out.view(np.uint32), rec.view(np.uint32))
                st = out[:, 2]
                print(json.dumps(dict(base, entry="match_ncc_pyramid_any", levels=L, npeaks=npeaks, path=ctx.last_path(),
                                      first_call_ms_wall=first_ms, **r,
                                      status={"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()), "-3": int((st == -3).sum()),
                                              "-4": int((st == -4).sum()), "nan": int(np.isnan(st).sum())})), flush=True)


if __name__ == "__main__":
    main()
