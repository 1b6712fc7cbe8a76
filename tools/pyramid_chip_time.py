#!/usr/bin/env python3
"""Time the coarse-to-fine exhaustive search at any chip size (mimc3_match_ncc_pyramid_chip) on BASELINE C2's pair and grid (200,000
points, R 15, centred on the a-priori shift), in ONE session beside its yardsticks:
    python3 tools/pyramid_chip_time.py [--pairs u8,dn12,dn16,float] [--levels 1,2,3] [--npeaks 0,4] [--reps K] [--tree LABEL]

    u8      the new entry at ocw 10, 16, 40, 80
    dn12    (C2 times 16 plus 4 random low bits) the new entry at ocw 10, 16, 40, 80; match_ncc_pyramid_dn at all six built sizes, and the
            new entry there too; the single-level match_ncc_full_chip_planes pass at each ocw
    dn16    (full low-order entropy) and
    float   (C2 times 0.37: non-integral) the new entry at ocw 10 beside the single-level match_ncc_full_chip pass

One JSON line per (pair, entry, ocw, levels, npeaks): the device time of a whole pass (HIP events through the context's timing hooks
around the _dev entry) -- median, mean, min and max of K passes after 2 warm-ups; min and max are what the mode-0 rule for a
scaled-integer pair at the six compares (search.cpp, pyramid_chip_u16_at_six: every pass of the new entry's series faster than every
pass of match_ncc_pyramid_dn's, at every level count and npeaks measured).  The last line is that verdict per ocw.
Test / tuning infrastructure."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mimc3_amd import api, synth  # noqa: E402
from hipmem import DevArray  # noqa: E402

SIX = (7, 15, 16, 30, 32, 40)
CHIP_OCW = (10, 16, 40, 80)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def low_bits(img, bits, seed):
    low = np.random.default_rng(seed).integers(0, 1 << bits, img.shape).astype(np.float32)
    return np.ascontiguousarray(np.where(img == 0, np.float32(0), img * np.float32(1 << bits) + low).astype(np.float32))


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
    pairs = arg("--pairs", "u8,dn12,dn16,float").split(",")
    levels = [int(v) for v in arg("--levels", "1,2,3").split(",")]
    npk = [int(v) for v in arg("--npeaks", "0,4").split(",")]
    reps = int(arg("--reps", "5"))
    c = synth.make_case("C2")
    R = 15
    shift = api.prior_shift(c.xyuvav, c.dt, c.mpp)
    base = {"tree": arg("--tree", ""), "case": "C2", "n": c.n, "radius": R, "reps": reps}
    d_xy, d_sh = DevArray(src=np.ascontiguousarray(c.xyuvav)), DevArray(src=shift)
    d_out, d_so, d_cand = DevArray((c.n, 8), np.float32), DevArray((c.n, 2), np.int32), DevArray((8, c.n, 3), np.float32)
    series = {}                                     # (entry, ocw) -> [(min, max)] over levels x npeaks, on dn12

    def emit(ctx, pair, entry, ocw, L, npeaks, call):
        r = timed(ctx, reps, call)
        st = d_out.numpy()[:, 2]
        print(json.dumps(dict(base, pair=pair, entry=entry, ocw=ocw, levels=L, npeaks=npeaks, path=ctx.last_path(), **r,
                              status={"ok": int((st >= -1).sum()), "-2": int((st == -2).sum()), "-3": int((st == -3).sum()),
                                      "-4": int((st == -4).sum()), "nan": int(np.isnan(st).sum())})), flush=True)
        if pair == "dn12" and L > 1:
            series.setdefault((entry, ocw), []).append((r["pass_ms_min"], r["pass_ms_max"]))

    def pyramid(ctx, pair, entry, ocw):
        fn = getattr(ctx, entry + "_dev")
        kw = {"mode": 0} if entry == "match_ncc_pyramid_chip" else {}
        for L in levels:
            for npeaks in npk:
                emit(ctx, pair, entry, ocw, L, npeaks,
                     lambda: fn(d_xy.ptr, c.n, c.offset, ocw, R, L, npeaks, d_out.ptr, d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr,
                                d_shift_out=d_so.ptr, **kw))

    def single(ctx, pair, entry, ocw, mode):
        fn = getattr(ctx, entry + "_dev")
        for npeaks in npk:
            emit(ctx, pair, entry, ocw, 0, npeaks,
                 lambda: fn(d_xy.ptr, c.n, c.offset, ocw, R, npeaks, d_out.ptr, d_cand.ptr if npeaks else 0, d_shift=d_sh.ptr, mode=mode))

    for pair in pairs:
        i0, i1 = {"u8": lambda: (c.i0, c.i1), "dn12": lambda: (low_bits(c.i0, 4, 5), low_bits(c.i1, 4, 6)),
                  "dn16": lambda: (low_bits(c.i0, 8, 5), low_bits(c.i1, 8, 6)),
                  "float": lambda: (np.ascontiguousarray(c.i0 * np.float32(0.37)), np.ascontiguousarray(c.i1 * np.float32(0.37)))}[pair]()
        with api.Context(0) as ctx:
            ctx.set_images(i0, i1)
            ctx.match_ncc_pyramid_chip(c.xyuvav[:8], c.offset, 10, R, max(levels), shift=shift[:8])     # (planes, tables, levels, first loads)
            ctx.enable_timing(True)
            if pair in ("u8", "dn12"):
                for ocw in CHIP_OCW:
                    pyramid(ctx, pair, "match_ncc_pyramid_chip", ocw)
                    if pair == "dn12":
                        single(ctx, pair, "match_ncc_full_chip_planes", ocw, 1)
                if pair == "dn12":
                    for ocw in SIX:
                        pyramid(ctx, pair, "match_ncc_pyramid_dn", ocw)
                        if ocw not in CHIP_OCW:
                            pyramid(ctx, pair, "match_ncc_pyramid_chip", ocw)
            else:
                pyramid(ctx, pair, "match_ncc_pyramid_chip", 10)
                single(ctx, pair, "match_ncc_full_chip", 10, 1)
    if "dn12" in pairs:
        verdict = {}
        for ocw in SIX:
            new, old = series.get(("match_ncc_pyramid_chip", ocw)), series.get(("match_ncc_pyramid_dn", ocw))
            if new and old:
                verdict[ocw] = all(a[1] < b[0] for a, b in zip(new, old))       # (configuration by configuration: same levels, same npeaks)
        print(json.dumps(dict(base, verdict="scaled-integer pair, mode 0 at the six: every pass of the matrix-core series faster than every "
                                            "pass of match_ncc_pyramid_dn's (levels > 1)", stays_on_matrix_cores=verdict)), flush=True)


if __name__ == "__main__":
    main()
