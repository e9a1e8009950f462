"""Two stages that share ONE kernel with different dynamic-LDS sizes, used alternately (luaradio_amd/csrc/launch_prep.h).

A kernel's dynamic-LDS limit above 48 KB is an attribute of the kernel, not of the stage that launches it.  While every stage set it to its own
size, a second stage that needs less lowered it below what the first one goes on launching with; kernel_allow_lds() only ever raises it.

Both stages below are FirForm::DecimLds1 (complex taps, decimation above 5, taps + 255 <= 6144) and launch fir_decim_lds_kernel<2, false, true>.
From launch_decim_lds: OW = min(256, (6144 - M) / D + 1) = 256 for both, span = 255 D + M, and
LDS floats = ((2 M + 3) & ~3) + 2 (span + (span >> 5) + 2):
  A: 1000 taps, D = 20: span 6100, 2000 + 2 (6100 + 190 + 2) = 14 584 floats = 58 336 bytes
  B:  300 taps, D = 22: span 5910,  600 + 2 (5910 + 184 + 2) = 12 792 floats = 51 168 bytes
Both exceed 49 152 and A's is the larger, so B's first launch is the one that would lower the limit under A's second.

Measured on an MI355X with the library as it was before launch_prep.h (each stage setting its own size): this test passes there too.  The ROCm
runtime in use does not hold a launch to a limit that was lowered after it had been raised, so the hazard was latent, not a live launch failure;
the test keeps it from becoming one under a runtime that does."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import types
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def make(cls, args, x):
    blk = cls(*args)
    blk.rate = 2.0
    blk.differentiate([types.type_of(x)])
    blk.initialize()
    return blk


def rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


def test_two_stages_share_a_kernel_with_different_lds_sizes():
    rng = np.random.default_rng(4120)
    n, cut = 13000, 6001          # 650 / 591 outputs: about 2.5 tiles of 256, two chunks per stage
    stages = []
    for ntaps, decim in ((1000, 20), (300, 22)):
        x = rand_c(rng, n)
        taps = (rand_c(rng, ntaps) / ntaps).astype(np.complex64)
        chain = lr.Chain([make(lr.FIRFilterBlock, [taps], x), make(lr.DownsamplerBlock, [decim], x)])
        stages.append((chain, x, O.FIR(taps, True, O.MODE_FMA).process(x)[::decim]))
    (a, xa, want_a), (b, xb, want_b) = stages
    # A, B, A, B
    a1 = a.process(xa[:cut])
    b1 = b.process(xb[:cut])
    a2 = a.process(xa[cut:])
    b2 = b.process(xb[cut:])
    got_a, got_b = np.concatenate([a1, a2]), np.concatenate([b1, b2])
    assert len(got_a) == len(want_a) and len(got_b) == len(want_b)
    assert np.array_equal(got_a, want_a)
    assert np.array_equal(got_b, want_b)
