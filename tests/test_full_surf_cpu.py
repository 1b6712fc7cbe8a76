"""CPU: the interface of the surfaces from the integer-class kernels (mimc3_match_ncc_full_surf, mimc3_stack_add_class and their _dev
twins), and what that interface promises, on the oracles alone: the float oracle's surface of an 8-bit, 12-bit or 16-bit pair, put
through the numpy stack as one layer, gives the record and the candidates of that class's integer oracle -- so "the class kernel's
record with the float kernel's surface" asks nothing the oracles disagree on.  Also: the null fixtures of the GPU tests hold at least
two points of every form of every kernel (counted from the images, the offset and the shift)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import assert_bits_equal
from full_any_common import full_any
from full_dn_common import full_dn
from full_multi_common import full_multi
from full_search_common import assert_records_match, full_search
from full_surf_common import BITS, NULL_GRID, SURF_OCW, SURF_R, class_counts, every_form_stores, null_classes, surf_case
from stack_common import NumpyStack, refused_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"mimc3_match_ncc_full_surf": 12, "mimc3_match_ncc_full_surf_dev": 14, "mimc3_stack_add_class": 6, "mimc3_stack_add_class_dev": 8}


def test_symbols_declared_and_exported():
    """The entries exist, with the argument counts of the header (and the Python binding's)."""
    from mimc3_amd import api
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mimc3_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "mimc3_amd", "csrc", "libmimc3_hip.so"))
    for s, nargs in SYMS.items():
        m = re.search(r"\bint(?:32_t)?\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, f"{s} is not declared in mimc3_hip.h"
        assert len(m.group(1).split(",")) == nargs, s
        assert hasattr(lib, s), f"{s} is not exported by libmimc3_hip.so"
        assert len(getattr(api._lib, s).argtypes) == nargs, s
    for name in ("match_ncc_full_surf", "match_ncc_full_surf_dev", "stack_add_class", "stack_add_class_dev"):
        assert callable(getattr(api.Context, name)), name


def integer_oracle(bits, i0, i1, xy, off, ocw, radius, npeaks, shift, swap):
    """Record (npeaks 0) and candidates of the class's integer oracle"""
    if bits == 16:
        return full_dn(i0, i1, xy, off, ocw, radius, 0, shift=shift, swap=swap)[0], full_dn(i0, i1, xy, off, ocw, radius, npeaks, shift=shift, swap=swap)[1]
    return full_search(i0, i1, xy, off, ocw, radius, shift=shift, swap=swap), full_multi(i0, i1, xy, off, ocw, radius, npeaks, shift=shift, swap=swap)[1]


@pytest.mark.parametrize("ocw,radius", [(7, 4), (16, 15), (40, 1)])
@pytest.mark.parametrize("bits", BITS)
def test_definition_on_the_oracles(bits, ocw, radius):
    """One layer of the float oracle's surface through NumpyStack == the integer oracle's record and candidates (the SNR within 1 ulp:
    its squares are added in another order)"""
    c, i0, i1, shift = surf_case(bits, ocw, True, radius)
    npeaks = 4
    for swap in (False, True):
        sgn = -1 if swap else 1
        off, sh = sgn * c.offset, sgn * shift
        rec_f, _, surf, _ = full_any(i0, i1, c.xyuvav, off, ocw, radius, 0, shift=sh, swap=swap)
        st = NumpyStack(c.n, radius, sh).add(surf, refused_of(rec_f))
        rec, cand, lay, mean = st.finish(npeaks, 1)
        want_rec, want_cand = integer_oracle(bits, i0, i1, c.xyuvav, off, ocw, radius, npeaks, sh, swap)
        what = f"{bits}-bit ocw {ocw} R {radius} swap {swap}"
        assert_bits_equal(mean, surf, what + ": one layer's mean is the layer")
        assert_records_match(rec, want_rec, what + ": record")
        assert_bits_equal(cand, want_cand, what + ": candidates")
        assert np.array_equal(lay == 0, want_rec[:, 2] == -3), what
        assert np.isnan(surf[want_rec[:, 2] == -3]).all()
        assert (want_rec[:, 2] >= -1).sum() >= c.n // 2              # (not a comparison of NaNs alone)


@pytest.mark.parametrize("ocw", SURF_OCW)
def test_null_fixtures_reach_every_form(ocw):
    """The GPU tests' null fixtures: >= 2 points without nulls, with nulls in the box only and with nulls in the chip, at every radius,
    both ways round (the nulls of the 12- and 16-bit fixtures are the 8-bit fixture's)"""
    for radius in SURF_R:
        for bits in BITS:
            c, i0, i1, shift = surf_case(bits, ocw, True, radius)
            for swap in (False, True):
                sgn = -1 if swap else 1
                cls = null_classes(i0, i1, c.xyuvav, sgn * c.offset, sgn * shift, ocw, radius, swap)
                assert every_form_stores(bits, cls), (NULL_GRID[ocw], bits, radius, swap, class_counts(cls))
                assert min(class_counts(cls)) >= 2, (NULL_GRID[ocw], bits, radius, swap, class_counts(cls))
            if bits == 8:
                c0, j0, j1, sh0 = surf_case(bits, ocw, False, radius)
                assert class_counts(null_classes(j0, j1, c0.xyuvav, c0.offset, sh0, ocw, radius))[1:] == (0, 0)
