#!/usr/bin/env python3
"""NCC stacking on a synthetic series: pairs that saw one motion under independent noise, and one pair at several chip sizes.
  python3 tools/stack_demo.py [--pairs 6] [--noise 100] [--radius 4] [--class]

Prints, per layer and for the stack, how many of the 60 grid points are misplaced (no fit, or a fit more than 0.5 px from the truth):
  series   one layer per pair at ocw 7 (the fixture of tests/test_stack_cpu.py, here through the device entries);
  chips    the first pair at ocw 15, 16 and 30 in one stack;
  both     every pair at every chip size.
--class builds the stacks through stack_add_class (the layers from the kernel of the pair's class: the same state, so the same counts).
Test / demonstration infrastructure."""
import os
import sys

ROOT = os.environ.get("MIMC3_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mimc3_amd import api  # noqa: E402
from full_fb_common import FB_OFFSET  # noqa: E402
from full_planes_time import arg  # noqa: E402
from stack_common import SERIES_NOISE_DN, SERIES_PAIRS, SERIES_R, SERIES_TRUTH, misplaced, series_pairs, series_points  # noqa: E402


def run(ctx, name, pairs, ocws, xy, shift, radius, cls=False):
    ctx.stack_begin(xy.shape[0], radius, shift)
    per = []
    for i0, i1 in pairs:
        ctx.set_images(i0, i1)
        for ocw in ocws:
            rec, _ = ctx.match_ncc_full_any(xy, FB_OFFSET, ocw, radius, 0, shift=shift, mode=1)
            per.append(int(misplaced(rec, SERIES_TRUTH).sum()))
            (ctx.stack_add_class if cls else ctx.stack_add)(xy, FB_OFFSET, ocw)
    rec, _, count = ctx.stack_finish()
    n, _, layers = ctx.stack_info()
    print(f"{name}: {layers} layers (ocw {list(ocws)}), misplaced of {n} per layer {per}, best layer {min(per)}, "
          f"stack {int(misplaced(rec, SERIES_TRUTH).sum())}", flush=True)


def main():
    npairs, noise, radius = int(arg("--pairs", SERIES_PAIRS)), int(arg("--noise", SERIES_NOISE_DN)), int(arg("--radius", SERIES_R))
    pairs = series_pairs(npairs, noise)
    xy, shift = series_points(30, radius)          # one grid for every chip size: the largest chip's margins
    cls = "--class" in sys.argv
    print(f"{npairs} pairs, one motion, +-{noise} DN of noise each; R {radius}; truth (du, dv) = {SERIES_TRUTH}"
          + ("; layers through stack_add_class" if cls else ""))
    with api.Context(0) as ctx:
        run(ctx, "series", pairs, (7,), xy, shift, radius, cls)
        run(ctx, "chips ", pairs[:1], (15, 16, 30), xy, shift, radius, cls)
        run(ctx, "both  ", pairs, (15, 16, 30), xy, shift, radius, cls)


if __name__ == "__main__":
    main()
