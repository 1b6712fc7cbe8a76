"""CPU: the stack beyond +-15 px by its definition (tests/stack_common.NumpyStack over the oracle's surfaces).

The definition does not depend on R: the central 31 x 31 block of an R-20 stack's mean is the mean of the R-15 layers, bit for bit.  The
chunk rule of mimc3_stack_chunk.  And what the feature is for: on a series displaced by (34, -27) px, out of reach of a 31 x 31 surface,
with +-100 DN of noise, the 81 x 81 surface of a single pair holds a decoy higher than the true peak at half of the points; the stack of
the series misplaces strictly fewer points than its best single layer."""
import numpy as np

from full_any_common import full_any
from full_fb_common import FB_OFFSET, fb_pair, fb_points
from stack_common import NumpyStack, misplaced, refused_of
from wide_common import FAR_TRUE

FAR_STACK_OCW, FAR_STACK_R, FAR_STACK_PAIRS, FAR_STACK_NOISE_DN = 7, 40, 5, 100


def test_central_block_of_an_r20_stack_is_the_r15_stack():
    xy, shift = fb_points(ocw=7, radius=15)
    n = xy.shape[0]
    wide, small = NumpyStack(n, 20, shift), NumpyStack(n, 15, shift)
    for k in range(3):
        i0, i1 = fb_pair(seed=41 + k)
        for ref in (wide, small):
            rec, _, surf, _ = full_any(i0, i1, xy, FB_OFFSET, 7, ref.radius, 0, shift=shift)
            ref.add(surf, refused_of(rec))
    both = (wide.lay == 3) & (small.lay == 3)                            # (the validity rule looks at the whole box, which differs)
    assert both.sum() >= 40
    for mc in (1, 3):
        block = wide.mean(mc).reshape(n, 41, 41)[:, 5:36, 5:36].reshape(n, 31 * 31)
        want = small.mean(mc)
        assert np.isfinite(want[both]).sum() > 30000
        assert block[both].tobytes() == want[both].tobytes(), f"min_count {mc}"


def test_stack_chunk_values():
    from mimc3_amd import api
    for r in range(-1, 50):
        want = 0 if r < 1 or r > 47 else 65536 if r <= 15 else (65536 * 961) // (2 * r + 1) ** 2
        assert api.stack_chunk(r) == want, r
    assert api.stack_chunk(15) == api.STACK_CHUNK and api.stack_chunk(16) == 57832 and api.stack_chunk(47) == 6978
    for r in range(16, 48):                                              # the layer scratch of R 15, and 32-bit cell indices
        assert api.stack_chunk(r) * (2 * r + 1) ** 2 <= 65536 * 961 < 2 ** 26


def far_series(pairs=FAR_STACK_PAIRS, noise_dn=FAR_STACK_NOISE_DN):
    """`pairs` 300 x 320 8-bit pairs that all moved by FAR_TRUE, each with its own texture and its own +-noise_dn DN of noise on image 1,
    and an 8 x 6 grid (tools/wide_stack_time.py prints the same counts on the device)"""
    from mimc3_amd import synth
    return [synth.make_small(seed=4800 + 17 * k, shift=FAR_TRUE, ocw=FAR_STACK_OCW, h=300, w=320, dimx=8, dimy=6, noise_dn=noise_dn, margin=70)
            for k in range(pairs)]


def test_stack_beats_every_single_layer_beyond_15_px():
    series = far_series()
    n = series[0].n
    ref = NumpyStack(n, FAR_STACK_R)
    per_layer = []
    for c in series:
        rec, _, surf, _ = full_any(c.i0, c.i1, c.xyuvav, (0, 0), FAR_STACK_OCW, FAR_STACK_R, 0)
        ref.add(surf, refused_of(rec))
        per_layer.append(int(misplaced(rec, FAR_TRUE).sum()))
    stacked = int(misplaced(ref.finish(0, 1)[0], FAR_TRUE).sum())
    print(f"R {FAR_STACK_R}, ocw {FAR_STACK_OCW}, +-{FAR_STACK_NOISE_DN} DN: misplaced per layer {per_layer}, stacked {stacked}, of {n} points")
    assert min(per_layer) > 0, "the noise level leaves the single layers something to get wrong"
    assert stacked < min(per_layer)
