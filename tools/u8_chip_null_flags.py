#!/usr/bin/env python3
"""tools/u8_chip_null_flags.py [config] -- CPU count for the chip-null skip of the register-tiled 8-bit kernel: over the
points of a BASELINE configuration (default C2) whose chip holds a null, at how many of the 19 dword task indices does the chip hold one?

The 33 x 33 chip of ocw 16 lives in 16 lanes: lane l owns rows l and l + 16 as nine dwords each (task index t = 9 * half + column,
t = 0..17) and lanes 0..8 own the nine dwords of row 32 (t = 18, one tail task).  Index t is flagged iff some dword of that index holds
a null among its valid bytes (chip column 32 is the single valid byte of a row's last dword).  No GPU needed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mimc3_amd import synth  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "C2"
    c = synth.make_case(name)
    ocw, cw = c.ocw, 2 * c.ocw + 1
    assert ocw == 16, "the task layout counted here is the 33-pixel chip's"
    z = np.zeros((c.i0.shape[0] + 1, c.i0.shape[1] + 1), np.int64)
    z[1:, 1:] = np.cumsum(np.cumsum(c.i0 == 0, axis=0), axis=1)
    u = c.xyuvav[:, 2].astype(np.int64) - ocw
    v = c.xyuvav[:, 3].astype(np.int64) - ocw

    def box(r0, r1, c0, c1):                               # nulls in chip rows r0..r1-1, columns c0..c1-1, per point
        return z[v + r1, u + c1] - z[v + r0, u + c1] - z[v + r1, u + c0] + z[v + r0, u + c0]

    nulls = box(0, cw, 0, cw)
    flags = np.zeros(len(u), np.int64)
    for t in range(18):
        half, col = divmod(t, 9)
        flags += box(16 * half, 16 * half + 16, 4 * col, min(4 * col + 4, cw)) > 0
    flags += box(32, 33, 0, cw) > 0
    sel = nulls > 0
    f = flags[sel]
    print("%s: %d points, %d with chip nulls" % (name, len(u), sel.sum()))
    print("flagged task indices per chip-null point: mean %.2f of 19, median %d, 90th percentile %d, maximum %d"
          % (f.mean(), np.median(f), np.percentile(f, 90), f.max()))
    print("share of the masked chip-side work done for dwords without a null: %.0f %%" % (100 * (1 - f.mean() / 19)))
    print("histogram (flagged indices: points):")
    for k, n in enumerate(np.bincount(f, minlength=20)):
        if n:
            print("  %2d: %6d" % (k, n))


if __name__ == "__main__":
    main()
