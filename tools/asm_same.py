#!/usr/bin/env python3
"""tools/asm_same.py old.s new.s -- are the kernels two device assembly listings share instruction-identical?

Both files are `hipcc ... --offload-arch=gfx950 --cuda-device-only -S` outputs of one source at two commits.  Per kernel (a global
function symbol with an .amdhsa_kernel descriptor) the instruction stream is compared with comments dropped and local labels
(.LBBn_m and friends) renumbered in order of first appearance, and so is the kernel descriptor (.amdhsa_* lines: registers, LDS,
scratch).  Prints one line per kernel of the old file -- same / DIFFERENT / missing -- then the kernels only the new file has, and
exits 1 unless every old kernel is there and the same.  No GPU needed."""
import re
import subprocess
import sys


def kernels(path):
    lines = open(path, errors="replace").read().splitlines()
    desc, cur = {}, None
    for ln in lines:                                     # the descriptors name the kernels
        t = ln.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = t.split()[1]; desc[cur] = []
        elif t.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and t:
            desc[cur].append(t)
    out, cur, body, labels = {}, None, [], {}
    lab_re = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
    for ln in lines:
        t = ln.split(";")[0].strip()
        if cur is None:
            if t.endswith(":") and t[:-1] in desc:
                cur, body, labels = t[:-1], [], {}
            continue
        if t.startswith(".Lfunc_end"):
            out[cur] = (body, desc[cur]); cur = None
            continue
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body.append(lab_re.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), t))
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.splitlines())) if p.returncode == 0 else {n: n for n in names}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    dm = demangle(sorted(set(old) | set(new)))
    short = lambda n: dm[n].replace("mimc3::", "").replace("void ", "")
    bad = 0
    for n in sorted(old, key=short):
        if n not in new:
            print("missing    %s" % short(n)); bad += 1
        elif old[n] == new[n]:
            print("same       %-80s %6d instructions" % (short(n), sum(1 for x in old[n][0] if not x.endswith(":"))))
        else:
            what = "instructions" if old[n][0] != new[n][0] else "descriptor"
            print("DIFFERENT  %s (%s)" % (short(n), what)); bad += 1
    for n in sorted(set(new) - set(old), key=short):
        print("new        %-80s %6d instructions" % (short(n), sum(1 for x in new[n][0] if not x.endswith(":"))))
    print("%d kernels of the old listing, %d the same, %d new" % (len(old), len(old) - bad, len(set(new) - set(old))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
