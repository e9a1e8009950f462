"""The RDS loopback: random frames as an FM broadcast multiplex at RF, and the reference topology of examples/rtlsdr_rds.lua:13-30 on the CPU.

Generator.  Frames -> bits (tests/helpers/rds_model.encode_frame) -> differential encoding e[i] = e[i-1] ^ b[i] -> two half symbols per e at
2375 Hz, (1, 0) for a 1 and (0, 1) for a 0, levels +-1 (what ManchesterDecoder and DifferentialDecoder undo) -> band-limited to +-2.4 kHz (the
spectrum set to zero above it) -> multiplex = pilot 0.1 sin(2 pi 19e3 t) + 0.05 d(t) cos(3 * 2 pi 19e3 t + theta) + an audio tone
0.3 sin(2 pi 1e3 t) -> FM at 75 kHz deviation, placed at +250 kHz, plus complex noise of 0.001 (as tests/test_gpu_pll.py builds its stereo signal).

Reference topology.  The oracle's block functions and the helper models, wired as tests/test_gpu_pll.py wires its two receivers.  The reference
samples the complex corrected signal at the clock recovered from its real part and then takes the real part; ClockSamplerModel on the real
part is the same thing."""
import functools

import numpy as np

from tests.helpers import rds_model

FS = 1102500.0
RF_N = 1 << 20
HALF_SYMBOL_RATE = 2375.0
NUM_FRAMES = 12


@functools.lru_cache(maxsize=None)
def sent_frames(seed=31, count=NUM_FRAMES):
    words = np.random.default_rng(seed).integers(0, 1 << 16, (count, 4)).astype(np.uint16)
    words.setflags(write=False)
    return words


def frame_bits(frames):
    return np.concatenate([rds_model.encode_frame([int(w) for w in f]) for f in frames])


def half_symbols(bits):
    """bits -> differentially encoded -> Manchester half-symbol levels +-1 (Float32)"""
    e = np.cumsum(np.asarray(bits, np.int64)) % 2                    # e[i] = e[i-1] ^ b[i], e[-1] = 0
    halves = np.stack([e, 1 - e], axis=1).reshape(-1)                # 1 -> (1, 0), 0 -> (0, 1)
    return (2.0 * halves - 1.0).astype(np.float32)


def data_track(levels, n, rate=FS, cutoff=2.4e3):
    """n samples of the half-symbol track at `rate`, band-limited to +-cutoff; past the last half symbol the track is 0"""
    k = (np.arange(n) * (HALF_SYMBOL_RATE / rate)).astype(np.int64)
    d = np.where(k < len(levels), levels.astype(np.float64)[np.minimum(k, len(levels) - 1)], 0.0)
    spec = np.fft.rfft(d)
    spec[np.fft.rfftfreq(n, 1 / rate) > cutoff] = 0
    return np.fft.irfft(spec, n)


@functools.lru_cache(maxsize=None)
def rds_signal(theta=0.0, n=RF_N, seed=31):
    """(ComplexFloat32 RF samples at FS, the frames sent)"""
    frames = sent_frames(seed)
    rng = np.random.default_rng(seed + 1)
    t = np.arange(n) / FS
    d = data_track(half_symbols(frame_bits(frames)), n)
    mpx = 0.1 * np.sin(2 * np.pi * 19e3 * t) + 0.05 * d * np.cos(3 * 2 * np.pi * 19e3 * t + theta) + 0.3 * np.sin(2 * np.pi * 1e3 * t)
    x = np.exp(1j * (2 * np.pi * 250e3 * t + 2 * np.pi * 75e3 / FS * np.cumsum(mpx)))
    x = (x + 0.001 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x.setflags(write=False)
    return x, frames


def _delay(x, k):
    return np.concatenate([np.zeros(k, x.dtype), x[:len(x) - k]])


def reference_bits(x, rate=FS, tune_offset=-250e3):
    """examples/rtlsdr_rds.lua:13-29 up to the differential decoder, from the oracle's blocks and the helper models"""
    import luaradio_amd as lr
    from luaradio_amd import types
    from oracle import oracle as O
    from tests.helpers import pll_model, phasecorr_model
    from tests.helpers.digital_model import ClockSamplerModel, DiffDecModel
    from tests.helpers.ert_model import ManchesterFast

    r1 = rate / 5
    demod = O.FMDiscriminator(1.25).process(O.tuner(tune_offset, 200e3, 5, rate, mode=O.MODE_LUA, rot_mode=O.MODE_F64).process(x))
    taps = types.Float32.vector_from_array(lr.filter_utils.fir_hilbert_transform(129, "hamming"))
    hilbert = (_delay(demod, 64) + 1j * O.FIR(taps, False).process(demod)).astype(np.complex64)
    delayed = _delay(hilbert, 129)
    pilot_taps = types.ComplexFloat32.vector_from_array(lr.filter_utils.firwin_complex_bandpass(129, [c / (r1 / 2) for c in (18e3, 20e3)]))
    pilot = O.FIR(pilot_taps, True).process(hilbert)
    pll_out = pll_model.run(pilot, 1500.0, 19e3 - 100, 19e3 + 100, 3.0, rate=r1)[0]
    baseband = O.lowpass(128, 4e3, r1, True).process(O.multiply_conjugate(delayed, pll_out))
    rrc_taps = types.Float32.vector_from_array(lr.filter_utils.fir_root_raised_cosine(101, r1, 1, 1 / 1187.5))
    shaped = O.FIR(rrc_taps, True).process(baseband)
    corrected = phasecorr_model.correct(shaped, 8000, form="lua")
    sliced = ClockSamplerModel(r1 / HALF_SYMBOL_RATE, 0.0, slice_t=0.0).process(np.ascontiguousarray(corrected.real))
    return DiffDecModel(False).process(ManchesterFast(False).process(sliced))


@functools.lru_cache(maxsize=None)
def reference_frames(theta=0.0):
    """the frames the CPU topology recovers from rds_signal(theta)"""
    got = rds_model.RDSFramerFast().process(reference_bits(rds_signal(theta)[0]))
    got.setflags(write=False)
    return got


def in_order(got, sent):
    """every row of `got` is a row of `sent`, in sending order (a subsequence)"""
    k = 0
    for row in np.asarray(got).reshape(-1, 4).tolist():
        while k < len(sent) and list(map(int, sent[k])) != row:
            k += 1
        if k == len(sent):
            return False
        k += 1
    return True
