"""The exact replay's shortcut on the GPU (match_mx_kernel.hip, match_px_kernel.hip): the fixtures that
tests/test_replay_shortcut_cpu.py qualifies, at ocw 7 and 16, on paths auto, u8px, u16 and f32, each with the shortcut on and off
(MIMC3_REPLAY_SHORTCUT=0): every output is the CPU oracle's bit for bit, with last_path() asserted, and the four outcome counts of
each kernel's diagnostics (MIMC3_MX_STATS, MIMC3_U8_STATS), read in a child process, are the ones the rule restated in numpy
predicts."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import replay_shortcut_common as rc
import test_mx_area_finish as af
from conftest import ROOT, assert_bits_equal

PATHS = (("auto", "u8_mfma"), ("u8px", "u8_exact"), ("u16", "u16_scaled"), ("f32", "f32_tiled"))
# where the register-tiled kernel has the shortcut (PxCfg::SHORTCUT): the 33-pixel chips of the three policies these paths take, and the
# 15-pixel chip of the 8-bit one
PX_SHORTCUT = {("auto", 7): True, ("u8px", 7): True, ("u16", 7): False, ("f32", 7): False,
               ("auto", 16): True, ("u8px", 16): True, ("u16", 16): True, ("f32", 16): True}
COUNT_RE = r"\[mimc3 (mx|u8) stats\] replay shortcut: taken with U empty (\d+), taken with U built (\d+), fell back (\d+), preconditions failed (\d+)"


def run_child(ocw, shortcut_on, outdir):
    """every fixture on every path in one child process with the diagnostics on; returns {(fixture, path): {"mx": counts, "u8": counts}}
    (the four counts summed over the call's launches of that kernel) and leaves the outputs in outdir/<fixture>_<path>.npy"""
    code = textwrap.dedent("""
        import sys, os
        sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
        import numpy as np
        from mimc3_amd import api
        import replay_shortcut_common as rc
        os.makedirs(%r, exist_ok=True)
        with api.Context(0) as ctx:
            for name, _ in rc.FIXTURES:
                i0, i1, xy, offset, off, uv, ocw = rc.fixture(name, %d)
                ctx.set_images(i0, i1)
                for path, want in %r:
                    sys.stderr.write("\\n[call %%s %%s]\\n" %% (name, path)); sys.stderr.flush()
                    ctx.set_path(path)
                    out = ctx.matching_ncc_dlc_2(xy, offset, off, uv, ocw)
                    assert ctx.last_path() == want, (name, path, ctx.last_path())
                    np.save(os.path.join(%r, "%%s_%%s.npy" %% (name, path)), out)
    """) % (ROOT, ROOT, outdir, ocw, PATHS, outdir)
    e = dict(os.environ, MIMC3_MX_STATS="1", MIMC3_U8_STATS="1", MIMC3_REPLAY_SHORTCUT="1" if shortcut_on else "0")
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    counts = {}
    for seg in r.stderr.split("\n[call ")[1:]:
        name, path = seg.split("]", 1)[0].split()
        c = {"mx": np.zeros(4, np.int64), "u8": np.zeros(4, np.int64)}
        for m in re.finditer(COUNT_RE, seg):
            c[m.group(1)] += np.array([int(v) for v in m.groups()[1:]], np.int64)
        counts[name, path] = c
    return counts


def predicted(name, ocw, path, want):
    """the four outcome counts of the matrix-core launch and of the register-tiled launch for one call, from the rule in numpy.  The
    matrix-core launch (path auto) reaches its replay with the clean and advance points whose every scan stays inside the area, and
    finishes those of them that af.stays_inside; the register-tiled launch reaches its replay with every other point whose grid is
    valid (the oracle's -3 marks the others)."""
    case = rc.fixture(name, ocw)
    pts = rc.fixture_points(name, ocw)
    a = af.areas(case)
    mx, px = np.zeros(4, np.int64), np.zeros(4, np.int64)
    for g, (val, climbs, start, _, oc) in enumerate(pts):
        done = False
        if path == "auto" and (a["clean"][g] or a["advance"][g]):
            c = np.array([c for centres, _, _ in climbs for c in centres], np.int64).reshape(-1, 2)
            rx, ry = c[:, 0] - a["tx"][g], c[:, 1] - a["ty"][g]
            if ((rx >= a["x0"][g] + 1) & (rx <= a["x1"][g] - 1) & (ry >= a["y0"][g] + 1) & (ry <= a["y1"][g] - 1)).all():
                mx[rc.OUTCOMES.index(oc)] += 1
                done = af.stays_inside(case, a, g)
        if not done and want[g, 2] != -3:
            px[rc.OUTCOMES.index(oc if PX_SHORTCUT[path, ocw] else "no_pre")] += 1
    return mx, px


@pytest.mark.gpu
@pytest.mark.parametrize("ocw", rc.OCWS)
def test_bits_and_outcome_counts(oracle, tmp_path, ocw):
    on = run_child(ocw, True, str(tmp_path / "on"))
    off = run_child(ocw, False, str(tmp_path / "off"))
    for name, _ in rc.FIXTURES:
        i0, i1, xy, offset, off_, uv, _ = rc.fixture(name, ocw)
        want = oracle.match(i0, i1, xy, offset, off_, uv, ocw)
        for path, _ in PATHS:
            for sw in ("on", "off"):
                assert_bits_equal(np.load(tmp_path / sw / f"{name}_{path}.npy"), want, f"ocw {ocw} {name} {path} shortcut {sw}")
            mx, px = predicted(name, ocw, path, want)
            got, got_off = on[name, path], off[name, path]
            print("ocw", ocw, name, path, "mx", got["mx"].tolist(), "predicted", mx.tolist(), "| px", got["u8"].tolist(), "predicted", px.tolist(),
                  "| off: mx", got_off["mx"].tolist(), "px", got_off["u8"].tolist())
            assert got["mx"].tolist() == mx.tolist(), (ocw, name, path, "matrix-core launch")
            assert got["u8"].tolist() == px.tolist(), (ocw, name, path, "register-tiled launch")
            # switched off: every point that reaches a replay counts as "preconditions failed"
            assert got_off["mx"].tolist() == [0, 0, 0, int(mx.sum())] and got_off["u8"].tolist() == [0, 0, 0, int(px.sum())], (ocw, name, path)
