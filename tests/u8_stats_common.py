"""Test infrastructure: the u8 matcher step's own statistic (MIMC3_MX_STATS), read from a child process -- shared by
tests/test_u8_step_lists.py and tests/test_value_limits.py."""
import os
import re
import subprocess
import sys
import textwrap

from conftest import ROOT

STATS_RE = (r"u8_classify: classes clean (\d+) rest (\d+) nulls (\d+) window-nulls (\d+); lists clean (\d+) rest (\d+)\n"
            r".*?clean: (\d+) points staged[^\n]*rest (\d+)")


def stats_run(body):
    """one forward call on path auto in a subprocess with the kernels' diagnostics on (the switch is read once per process):
    (classes clean, rest, nulls, window-nulls; list lengths clean, rest) as u8_classify left them, then the points the
    matrix-core launch finished and the points classed kMxRest after it"""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
        import numpy as np
        from mimc3_amd import api, synth
        import test_u8_step_lists as t
        %s
        with api.Context(0) as ctx:
            ctx.set_images(i0, i1)
            ctx.matching_ncc_dlc_2(xy, offset, off, uv, ocw)
            assert ctx.last_path() == "u8_mfma"
    """) % (ROOT, ROOT, body)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIMC3_MX_STATS="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(STATS_RE, r.stderr, re.S)
    assert m, r.stderr[-2000:]
    return tuple(int(v) for v in m.groups())
