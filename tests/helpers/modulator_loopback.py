"""The two noise-free loopback chains of the modulator tests, shared by the CPU model test and the GPU test: seeds, rates, filters, where the
receiver samples, and the decisions."""
import numpy as np

from luaradio_amd import filter_utils
from tests.helpers import modulator_model as mm

NBITS = 4000
QAM_SEED, PAM_SEED = 11, 12
SYMBOL_RATE = 1.0
RRC_TAPS, RRC_BETA = 129, 0.35


def rrc(period):
    """RootRaisedCosineFilterBlock's taps at `period` samples per symbol, as Float32"""
    return np.asarray(filter_utils.fir_root_raised_cosine(RRC_TAPS, period * SYMBOL_RATE, RRC_BETA, 1 / SYMBOL_RATE), np.float64).astype(np.float32)


def bits(seed):
    return np.random.default_rng(seed).integers(0, 2, NBITS).astype(np.uint8)


def pulse_peak(period):
    """(index, value) of the largest sample of one held symbol through both filters: where the receiver samples, and the gain it divides by"""
    h = rrc(period).astype(np.float64)
    p = np.convolve(np.convolve(np.ones(period), h), h)
    k = int(np.argmax(p))
    return k, float(p[k])


def qam_receiver_delay(period):
    """DelayBlock(d), d in 1 .. period, that moves the pulse peak onto a multiple of `period`, and the first symbol's index behind Downsampler(period)"""
    peak, _ = pulse_peak(period)
    d = (-peak) % period or period
    return d, (peak + d) // period


def nearest_points(samples, table):
    return np.argmin(np.abs(np.asarray(samples, np.complex128)[:, None] - np.asarray(table, np.complex128)[None, :]), axis=1)


def symbols_to_bits(values, nbits_per_symbol):
    """msb first, as the modulators pack them"""
    shifts = np.arange(nbits_per_symbol - 1, -1, -1)
    return ((np.asarray(values)[:, None] >> shifts) & 1).astype(np.uint8).reshape(-1)


def find_lag(decoded, sent, first, span=2):
    """the lag first .. first + span (in bits) with decoded[lag + k] == sent[k] for every k the two share, or None: the receiver's first `lag`
    decisions come from before the first symbol's pulse peak (the filters' group delay)"""
    for lag in range(first, first + span + 1):
        n = min(len(decoded) - lag, len(sent))
        if n > 0 and np.array_equal(decoded[lag:lag + n], sent[:n]):
            return lag
    return None
