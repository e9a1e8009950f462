"""Named, seeded, read-only ComplexFloat32 streams for the PLL tests (tests/test_pll_cpu.py plays them through the plan on the CPU,
tests/test_gpu_pll.py through the kernels): each is built to drive the speculate / verify / repair stage down one particular path, and the CPU
test asserts that it does before the GPU test relies on it.  Unless a docstring says otherwise: carrier 0.1003 cycles / sample (inside the unit-test
loop's 0.095 .. 0.105), phase 0.3, plus 0.1 complex noise, n = 2^16."""
import functools

import numpy as np

N = 1 << 16
LOOP = (0.01, 0.19, 0.21)              # loop bandwidth, frequency_min, frequency_max at rate 2.0: the loop of tests/test_gpu_pll.py
NEGATIVE_LOOP = (0.01, -0.21, -0.19)
PILOT_LOOP = (100, 18950, 19050)       # PLLBlock(100, 18950, 19050, 2) of the stereo and RDS receivers
PILOT_RATE = 220500.0
BURST = (30000, 32000)                 # the stretch `burst` and `gap` replace


def cnoise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def carrier(n, freq, phase=0.3):
    return np.exp(1j * (2 * np.pi * freq * np.arange(n) + phase))


def _frozen(x):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    x.setflags(write=False)
    return x


def _locked(n, seed):
    return carrier(n, 0.1003) + 0.1 * cnoise(n, seed)


@functools.lru_cache(maxsize=None)
def burst():
    """Lock, 2000 samples of unit complex noise, lock again: the verify pass rejects the segments of the burst and those behind it whose lanes
    warmed up inside it; the walk starts in the middle of the call, stops where the speculated entries agree again, and the rest stays speculated."""
    x = _locked(N, 31)
    x[BURST[0]:BURST[1]] = cnoise(BURST[1] - BURST[0], 32)
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def gap():
    """The same stretch set to exact 0 + 0j (a squelch): the detector sees atan2(+-0, +-0), which is pi where the product's real part is -0.  The
    zeros are the same for every lane, so inside the gap a segment is re-accepted from its speculated entry behind a repaired one."""
    x = _locked(N, 33)
    x[BURST[0]:BURST[1]] = 0
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def early_and_late():
    """n = 2^16 + 37.  Noise over samples 70 .. 699 rejects segment 1, the first one that is verified (its predecessor started from the carried
    state); noise over the last 500 samples makes the walk end in the last, partial segment (37 samples)."""
    n = N + 37
    x = _locked(n, 34)
    x[70:700] = cnoise(630, 35)
    x[n - 500:] = cnoise(500, 36)
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def jump():
    """The carrier's phase steps by 2 rad at sample 40003.  Every lane that sees the step has the same history before it, so nothing is rejected:
    the 4-launch path through a transient."""
    n = np.arange(N)
    x = np.exp(1j * (2 * np.pi * 0.1003 * n + 0.3 + 2.0 * (n >= 40003))) + 0.1 * cnoise(N, 37)
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def locked():
    """carrier plus 0.1 noise, nothing else: for the multipliers (-2: phi_multiplied runs negative; 20: more than a turn per sample)"""
    return _frozen(_locked(N, 38))


@functools.lru_cache(maxsize=None)
def negative():
    """The complex conjugate of `locked`, a carrier at -0.1003, for NEGATIVE_LOOP: phi_locked runs downward and wraps at -2 pi."""
    return _frozen(np.conj(_locked(N, 38)))


@functools.lru_cache(maxsize=None)
def clean_centre():
    """A carrier at exactly 0.1, the loop's centre, without noise: err sits in the Float32 rounding of the VCO sample, where two trajectories
    stop converging.  The input a SignalSource -> PLLBlock demonstration makes."""
    return _frozen(carrier(N, 0.1))


@functools.lru_cache(maxsize=None)
def clean_off():
    """The same at 0.1003, off the centre."""
    return _frozen(carrier(N, 0.1003))


@functools.lru_cache(maxsize=None)
def pilot():
    """19 000 Hz at 220 500 Hz plus 0.3 complex noise, for PILOT_LOOP with multiplier 2 (W = 5 957)."""
    return _frozen(carrier(N, 19000.0 / PILOT_RATE) + 0.3 * cnoise(N, 39))
