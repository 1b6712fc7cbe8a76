"""GPU: what the exhaustive-search family refuses, and with which code -- one table for every host entry and its _dev twin (the full
searches, forward-backward, the pyramids, the stack's layer adds), single faults and pairs of faults whose order decides the code.

The expected codes are literals, recorded from a run of this file on the commit before the host layer was given one shape (call
descriptor, rules, one check, one launch); they are not derived from the code under test.  Where two faults meet, the code is whichever
rule the library makes first, and the table pins that order.  After every group of refusals one valid call returns the bytes it returned
before them.  The functions are taken from api._lib by name with pointer-typed prototypes of the test's own, so that a null can be
passed where api.py's prototypes want an array."""
import ctypes as C

import numpy as np
import pytest

import hipmem
from conftest import assert_bits_equal
from full_any_common import to_float
from full_dn_common import to_dn16
from hipmem import DevArray
from mimc3_amd import synth

pytestmark = pytest.mark.gpu

# include/mimc3_hip.h
MIMC3_EINVAL, MIMC3_EBOUNDS, MIMC3_ESTATE, MIMC3_EUNSUPPORTED = -1, -2, -5, -6

OCW, R, STACK_R, SURF_R, MAX_PEAKS = 7, 5, 5, 16, 9

# the arguments of every host entry, in order; its _dev twin takes (off_u, off_v) for `off` and a stream at the end
SIGS = {
    "full": "h xy n off shift ocw R swap out",
    "full_multi": "h xy n off shift ocw R npeaks swap out cand",
    "full_planes": "h xy n off shift ocw R npeaks swap out cand",
    "full_dn": "h xy n off shift ocw R npeaks swap out cand",
    "full_any": "h xy n off shift ocw R npeaks swap mode out cand surf",
    "wide": "h xy n off shift ocw R npeaks swap out cand surf",
    "full_fb": "h xy n off shift ocw R npeaks mode out cand fb",
    "wide_fb": "h xy n off shift ocw R npeaks out cand fb",
    "pyramid": "h xy n off shift ocw R levels swap out shift_out",
    "pyramid_dn": "h xy n off shift ocw R levels npeaks swap out cand shift_out",
    "pyramid_any": "h xy n off shift ocw R levels npeaks swap mode out cand shift_out",
    "stack_add": "h xy n off ocw swap",
    "stack_add_scaled": "h xy n off ocw R swap scale weight",
}
POINTERS = {"h", "xy", "off", "shift", "out", "cand", "surf", "fb", "shift_out", "stream"}
DOUBLES = {"scale", "weight"}

ALL = tuple(SIGS)
STACK = ("stack_add", "stack_add_scaled")
PYR = ("pyramid", "pyramid_dn", "pyramid_any")
SEARCH = tuple(e for e in ALL if e not in STACK)
WIDE = ("wide", "wide_fb", "stack_add_scaled")                      # R up to mimc3_wide_max_radius(ocw)
R15 = tuple(e for e in SEARCH if e not in WIDE)
NPK = tuple(e for e in SEARCH if "npeaks" in SIGS[e])
MODE = tuple(e for e in ALL if "mode" in SIGS[e])
FB = ("full_fb", "wide_fb")
U8_ONLY = ("full", "full_multi", "pyramid")
ACCEPTS = {e: ("u8",) for e in U8_ONLY}
ACCEPTS.update(full_planes=("u8", "u16"), full_dn=("u8", "u16", "dn16"), pyramid_dn=("u8", "u16", "dn16"))

BUF = "buf"         # an override: the entry's own buffer for that argument
BAD_CHIP = "bad"    # an override of xy: point 3's chip leaves the image (host entries)
BIG = (1 << 24) + 1

# (what, pair, overrides, entries, code of the host entry, code of the _dev twin); a code of None: that twin is not called.
# `off` is the offset (host: the array; _dev: off_u, off_v).  The pair "none" is a context without images.
ROWS = [
    # ---- single faults ----
    ("N = 0", "u8", dict(n=0), ALL, MIMC3_EINVAL, MIMC3_EINVAL),
    ("xyuvav null", "u8", dict(xy=None), ALL, MIMC3_EINVAL, MIMC3_EINVAL),
    ("out null", "u8", dict(out=None), SEARCH, MIMC3_EINVAL, MIMC3_EINVAL),
    ("offset null", "u8", dict(off=None), ALL, MIMC3_EINVAL, None),
    ("ocw 8", "u8", dict(ocw=8), ALL, MIMC3_EINVAL, MIMC3_EINVAL),
    ("R 0", "u8", dict(R=0), SEARCH + ("stack_add_scaled",), MIMC3_EINVAL, MIMC3_EINVAL),
    ("R 16", "u8", dict(R=16), R15, MIMC3_EINVAL, MIMC3_EINVAL),
    ("R wide_max_radius + 1", "u8", dict(R="wmax+1"), WIDE, MIMC3_EINVAL, MIMC3_EINVAL),
    ("npeaks 9", "u8", dict(npeaks=9, cand=BUF), NPK, MIMC3_EINVAL, MIMC3_EINVAL),
    ("npeaks 2, no cand", "u8", dict(npeaks=2, cand=None), NPK, MIMC3_EINVAL, MIMC3_EINVAL),
    ("cand with npeaks 0", "u8", dict(npeaks=0, cand=BUF), NPK, MIMC3_EINVAL, MIMC3_EINVAL),
    ("mode 2", "u8", dict(mode=2), MODE, MIMC3_EINVAL, MIMC3_EINVAL),
    ("mode -1", "u8", dict(mode=-1), MODE, MIMC3_EINVAL, MIMC3_EINVAL),
    ("no images", "none", dict(), ALL, MIMC3_ESTATE, MIMC3_ESTATE),
    ("a scaled-integer pair", "u16", dict(), U8_ONLY, MIMC3_EUNSUPPORTED, MIMC3_EUNSUPPORTED),
    ("a 16-bit-DN pair", "dn16", dict(), U8_ONLY + ("full_planes",), MIMC3_EUNSUPPORTED, MIMC3_EUNSUPPORTED),
    ("a float pair", "float", dict(), U8_ONLY + ("full_planes", "full_dn", "pyramid_dn"), MIMC3_EUNSUPPORTED, MIMC3_EUNSUPPORTED),
    ("surfaces of an integer kernel", "u8", dict(surf=BUF), ("full_any",), MIMC3_EINVAL, MIMC3_EINVAL),
    ("fb null", "u8", dict(fb=None), FB, MIMC3_EINVAL, MIMC3_EINVAL),
    ("levels 0", "u8", dict(levels=0), PYR, MIMC3_EINVAL, MIMC3_EINVAL),
    ("levels 6", "u8", dict(levels=6), PYR, MIMC3_EINVAL, MIMC3_EINVAL),
    ("coarsest level smaller than a chip", "u8", dict(levels=5), PYR, MIMC3_EINVAL, MIMC3_EINVAL),     # 160 >> 4 = 10 < 15
    ("chip outside the image", "u8", dict(xy=BAD_CHIP), ALL, MIMC3_EBOUNDS, None),
    ("box beyond the zero border", "u8", dict(off=(300, 0)), tuple(e for e in ALL if e not in PYR), MIMC3_EBOUNDS, None),
    ("starting displacement beyond 2^24", "u8", dict(off=(BIG, 0)), PYR, MIMC3_EINVAL, None),
    # ---- pairs of faults: the first rule made decides ----
    ("class + R 16", "u16", dict(R=16), U8_ONLY, MIMC3_EINVAL, MIMC3_EINVAL),
    ("class + R 16", "dn16", dict(R=16), ("full_planes",), MIMC3_EINVAL, MIMC3_EINVAL),
    ("class + R 16", "float", dict(R=16), ("full_dn", "pyramid_dn"), MIMC3_EINVAL, MIMC3_EINVAL),
    ("class + box beyond the border", "u16", dict(off=(300, 0)), ("full", "full_multi"), MIMC3_EUNSUPPORTED, None),
    ("class + box beyond the border", "dn16", dict(off=(300, 0)), ("full_planes",), MIMC3_EUNSUPPORTED, None),
    ("class + box beyond the border", "float", dict(off=(300, 0)), ("full_dn",), MIMC3_EUNSUPPORTED, None),
    ("class + chip outside", "float", dict(xy=BAD_CHIP), U8_ONLY + ("full_planes", "full_dn", "pyramid_dn"), MIMC3_EUNSUPPORTED, None),
    ("no images + ocw 8", "none", dict(ocw=8), ALL, MIMC3_EINVAL, MIMC3_EINVAL),
    # (the entries older than `mode` take none; on the entries that do, no class is refused, so a bad mode is the only fault left)
    ("mode 2 on a float pair", "float", dict(mode=2), MODE, MIMC3_EINVAL, MIMC3_EINVAL),
    ("mode 2 + surfaces of an integer kernel", "u8", dict(mode=2, surf=BUF), ("full_any",), MIMC3_EINVAL, MIMC3_EINVAL),
    ("surfaces of an integer kernel + box beyond the border", "u8", dict(surf=BUF, off=(300, 0)), ("full_any",), MIMC3_EBOUNDS, None),
    # (host entry and _dev twin differ here, and have since the entries were added: recorded as they are)
    ("no images + mode 2", "none", dict(mode=2), ("full_any", "full_fb"), MIMC3_ESTATE, MIMC3_EINVAL),
    ("no images + mode 2", "none", dict(mode=2), ("pyramid_any",), MIMC3_ESTATE, MIMC3_ESTATE),
    ("no images + fb null", "none", dict(fb=None), FB, MIMC3_ESTATE, MIMC3_EINVAL),
    ("class + coarsest level smaller than a chip", "float", dict(levels=5), ("pyramid", "pyramid_dn"), MIMC3_EUNSUPPORTED, MIMC3_EUNSUPPORTED),
    ("npeaks 9 + ocw 8", "u8", dict(npeaks=9, cand=BUF, ocw=8), NPK, MIMC3_EINVAL, MIMC3_EINVAL),
    ("chip outside + levels 6", "u8", dict(xy=BAD_CHIP, levels=6), PYR, MIMC3_EINVAL, None),
    ("chip outside + box beyond the border", "u8", dict(xy=BAD_CHIP, off=(300, 0)), tuple(e for e in ALL if e not in PYR), MIMC3_EBOUNDS, None),
]
PAIRS = ("u8", "u16", "dn16", "float", "none")


@pytest.fixture(scope="module")
def api():
    from mimc3_amd import api as a
    return a


def entry_fn(api, name, dev):
    sym = ("mimc3_" if name in STACK else "mimc3_match_ncc_") + name + ("_dev" if dev else "")
    names = SIGS[name].split()
    if dev:
        i = names.index("off")
        names = names[:i] + ["off_u", "off_v"] + names[i + 1:] + ["stream"]
    fn = api._lib[sym]                       # (a fresh function object: api.py's own prototypes stay as they are)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p if a in POINTERS else C.c_double if a in DOUBLES else C.c_int32 for a in names]
    return fn, names


class Pair:
    """one context with one pair resident (or none), and the buffers of a call on it: host arrays and device arrays"""

    def __init__(self, api, case, kind, images):
        self.kind, self.images = kind, images
        self.ctx = api.Context(0)
        if images is not None:
            self.ctx.set_images(*images)
        self.n = n = case.n
        bad = case.xyuvav.copy()
        bad[3, 2] = 3.0
        self.host = dict(xy=np.ascontiguousarray(case.xyuvav, np.float64), bad=np.ascontiguousarray(bad, np.float64),
                         out=np.zeros((n, 8), np.float32), cand=np.zeros((MAX_PEAKS, n, 3), np.float32),
                         surf=np.zeros((n, (2 * SURF_R + 1) ** 2), np.float32), fb=np.zeros((1 + MAX_PEAKS, n, 4), np.float32),
                         shift_out=np.zeros((n, 2), np.int32))
        self.dev = {k: DevArray(src=v) for k, v in self.host.items() if k != "bad"}
        self.keep = []

    def pointer(self, key, dev):
        return self.dev[key].ptr if dev else self.host[key].ctypes.data

    def call(self, api, name, dev, over=None):
        """the entry (or its _dev twin) with valid arguments, changed by `over` -> its return code"""
        fn, names = entry_fn(api, name, dev)
        over = dict(over or {})
        if over.get("R") == "wmax+1":
            over["R"] = api.wide_max_radius(over.get("ocw", OCW)) + 1
        p = dict(h=self.ctx._h, n=self.n, shift=None, ocw=OCW, R=R, npeaks=2 if name == "full_multi" else 0, swap=0, mode=0, levels=2,
                 scale=1.0, weight=1.0, stream=None, surf=None, off=(0, 0))
        for key in ("xy", "out", "fb", "shift_out"):
            p[key] = self.pointer(key, dev)
        p.update(over)
        if "cand" not in over:
            p["cand"] = BUF if p["npeaks"] > 0 else None
        for key in ("cand", "surf"):
            if p[key] == BUF:
                p[key] = self.pointer(key, dev)
        if p["xy"] == BAD_CHIP:
            assert not dev
            p["xy"] = self.host["bad"].ctypes.data
        if p["off"] is not None:
            p["off_u"], p["off_v"] = p["off"]
            off = np.asarray(p["off"], np.int32)
            self.keep = [off]
            p["off"] = off.ctypes.data
        return fn(*[p[a] for a in names])

    def probe(self, api, name, dev):
        """one valid call on this context -> its bytes: the entry's own where it takes the pair (the stack entries: a fresh stack, the
        layer, the finish), match_ncc_full_any where it does not; a context without images gets its stack and nothing else"""
        ctx = self.ctx
        if name in STACK or self.images is None:
            ctx.stack_begin(self.n, STACK_R)
        if self.images is None:
            return None
        if self.kind not in ACCEPTS.get(name, PAIRS):
            return [ctx.match_ncc_full_any(self.host["xy"], (0, 0), OCW, R, 0)[0]]
        assert self.call(api, name, dev) == 0, api._lib.mimc3_last_error()
        assert hipmem._hip.hipDeviceSynchronize() == 0
        if name in STACK:
            return [ctx.stack_finish(0)[0]]
        got = {k: (self.dev[k].numpy() if dev else self.host[k].copy()) for k in ("out", "cand", "fb", "shift_out")}
        n = self.n
        res = [got["out"]]
        if name == "full_multi":
            res.append(got["cand"].reshape(-1)[:2 * n * 3])
        if name in FB:
            res.append(got["fb"].reshape(-1)[:n * 4])
        if name in PYR:
            res.append(got["shift_out"].astype(np.float32))
        return res


@pytest.fixture(scope="module")
def world(api):
    c = synth.make_small(seed=21, ocw=OCW)
    images = dict(u8=(c.i0, c.i1),
                  u16=(np.ascontiguousarray(c.i0 * 16, np.float32), np.ascontiguousarray(c.i1 * 16, np.float32)),      # 12-bit DN
                  dn16=(to_dn16(c.i0, 1), to_dn16(c.i1, 2)), float=(to_float(c.i0, 1), to_float(c.i1, 2)), none=None)
    w = {}
    for kind in PAIRS:
        w[kind] = Pair(api, c, kind, images[kind])
    yield w
    for p in w.values():
        p.ctx.close()


def test_the_pairs_have_their_classes(api, world):
    want = dict(u8="u8_mfma_full", u16="u16_full", dn16="f32i_full", float="f32g_full")
    for kind, path in want.items():
        ctx = world[kind].ctx
        ctx.match_ncc_full_any(world[kind].host["xy"], (0, 0), OCW, R, 0)
        assert ctx.last_path() == path, kind


@pytest.mark.parametrize("name", ALL)
def test_refusals(api, world, name):
    rows = [r for r in ROWS if name in r[3]]
    assert rows
    wrong = []
    for kind in PAIRS:
        here = [r for r in rows if r[1] == kind]
        if not here:
            continue
        p = world[kind]
        for dev in (False, True):
            before = p.probe(api, name, dev)
            for what, _, over, _, host_code, dev_code in here:
                want = dev_code if dev else host_code
                if want is None:
                    continue
                got = p.call(api, name, dev, over)
                msg = api._lib.mimc3_last_error().decode(errors="replace")
                print(f"{name}{'_dev' if dev else ''} | {kind} | {what}: {got} (want {want}) {msg}")
                if got != want:
                    wrong.append((name, dev, kind, what, got, want, msg))
            after = p.probe(api, name, dev)
            for k, (a, b) in enumerate(zip(before or [], after or [])):
                assert_bits_equal(b, a, f"{name}{'_dev' if dev else ''} on the {kind} pair: the valid call after the refusals, item {k}")
    assert not wrong, wrong


def test_timing_comes_back(api, world):
    """The entries that suspend the context's timing flag around their inner searches (forward-backward, the pyramid, a stack add) time
    the whole call, and the flag is on again afterwards: a plain search right behind reports a time of its own."""
    p = world["u8"]
    ctx, xy = p.ctx, p.host["xy"]
    ctx.enable_timing(True)
    try:
        ctx.stack_begin(p.n, STACK_R)
        for what, call in (("full_fb", lambda: ctx.match_ncc_full_fb(xy, (0, 0), OCW, R, 2)),
                           ("pyramid_any", lambda: ctx.match_ncc_pyramid_any(xy, (0, 0), OCW, R, 2)),
                           ("stack_add", lambda: ctx.stack_add(xy, (0, 0), OCW))):
            call()
            whole = ctx.last_kernel_ms()
            ctx.match_ncc_full(xy, (0, 0), OCW, R)
            plain = ctx.last_kernel_ms()
            print(f"{what}: {whole:.4f} ms, match_ncc_full behind it {plain:.4f} ms")
            assert whole > 0 and plain > 0, what
        for mode in (0, 1):
            ctx.match_ncc_full_any(xy, (0, 0), OCW, R, 2, mode=mode)
            forward = ctx.last_path()
            ctx.match_ncc_full(xy, (0, 0), OCW, R)
            ctx.match_ncc_full_fb(xy, (0, 0), OCW, R, 2, mode=mode)
            assert ctx.last_path() == forward
    finally:
        ctx.enable_timing(False)
        ctx.stack_begin(0, 0)
