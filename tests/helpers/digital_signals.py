"""Synthetic signals for the digital receivers' functional tests (tests/test_gpu_phasecorr.py): each carries a known bit payload.

  afsk1200_fm   AX.25: NRZI-coded AFSK1200 (1200 / 2200 Hz, phase continuous), FM-modulated (3 kHz deviation) at -tune_offset
  fsk2_pocsag   POCSAG: 2-FSK, a 1 bit at -4.5 kHz (the mark filter of examples/rtlsdr_pocsag.lua), a 0 bit at +4.5 kHz, at -tune_offset
  dbpsk31       BPSK31: differential BPSK (a 0 bit reverses the phase), 31.25 baud, complex baseband, carrier phase `phase` plus a slow
                sinusoidal drift, additive complex Gaussian noise
"""
import numpy as np


def payload(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def framed(bits, seed, lead=256, trail=128):
    """random bits in front of and behind the payload (the receivers' filters and clock recovery settle on them)"""
    rng = np.random.default_rng(seed + 1)
    return np.concatenate([rng.integers(0, 2, lead), bits, rng.integers(0, 2, trail)]).astype(np.uint8)


def _symbol_track(levels, baud, rate):
    """per sample: the level of the symbol it falls in"""
    n = int(len(levels) * rate / baud)
    return levels[np.minimum((np.arange(n) * baud / rate).astype(np.int64), len(levels) - 1)]


def afsk1200_fm(bits, rate=1e6, tune_offset=-100e3, deviation=3e3):
    # NRZI (AX.25): a 0 bit changes the tone, a 1 bit keeps it - differentialdecoder(invert = true) undoes it
    tone = np.cumsum(1 - bits.astype(np.int64)) % 2
    f = np.where(_symbol_track(tone, 1200.0, rate) == 1, 1200.0, 2200.0)
    audio = np.cos(2 * np.pi * np.cumsum(f) / rate)
    phase = 2 * np.pi * np.cumsum(-tune_offset + deviation * audio) / rate
    return np.exp(1j * phase).astype(np.complex64)


def fsk2_pocsag(bits, rate=1e6, tune_offset=-100e3, baud=1200.0, shift=4.5e3):
    f = np.where(_symbol_track(bits, baud, rate) == 1, -shift, shift)
    phase = 2 * np.pi * np.cumsum(-tune_offset + f) / rate
    return np.exp(1j * phase).astype(np.complex64)


def dbpsk31(bits, rate=1000.0, phase=1.2, drift=0.2, noise=0.0, seed=0):
    sym = np.cumprod(np.where(bits == 1, 1.0, -1.0))          # a 0 bit reverses the phase
    s = _symbol_track(sym, 31.25, rate)
    n = len(s)
    theta = phase + drift * np.sin(2 * np.pi * np.arange(n) / n)
    rng = np.random.default_rng(seed)
    w = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    return (s * np.exp(1j * theta) + w).astype(np.complex64)


def contains(out, bits, skip=64):
    """the payload appears contiguously in the receiver's output after its first `skip` bits"""
    out = np.asarray(out, np.uint8)[skip:]
    if len(out) < len(bits):
        return False
    hay, needle = out.tobytes(), np.asarray(bits, np.uint8).tobytes()
    return hay.find(needle) >= 0
