"""What a streaming stage carries from one call to the next (luaradio_amd/csrc/stage_carry.h: a call reads in(), its kernels write out(), the
call flips once behind its last launch), one row per stage that keeps such a pair and per kernel form of it.  Two properties per row:

a. reset (and seek, where the stage has one of its own) after an ODD number of calls - the pair then sits on its second slot - gives the bytes
   of a freshly created stage;
b. ragged calls cut at 1, 2, tile - 1, tile and tile + 1 give what one call gives: byte for byte where the stage's own test says so, otherwise
   within exactly the bound of the test the row names.  Stages whose kernels walk a tile grid (align() > 1) are also cut on multiples of it,
   where the comparison is exact.

Shapes: two tiles of the stage's own tile size and a ragged tail, the smallest filter, window, code and channel count each stage takes."""
import collections
import functools

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from luaradio_amd import blocks as B
from luaradio_amd import filter_utils
from tests.helpers import iir_forms as F

pytestmark = pytest.mark.gpu

C, R, BIT, BYTE = types.ComplexFloat32, types.Float32, types.Bit, types.Byte


def make(cls, args, in_type, rate=2.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def rand(rng, n, t):
    if t is C:
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    if t is R:
        return rng.uniform(-1, 1, n).astype(np.float32)
    return rng.integers(0, 2 if t is BIT else 256, n).astype(np.uint8)


def levelled(rng, n, t):
    """a level that steps between -80 and -20 dBFS every 500 samples: across the squelch and AGC thresholds"""
    level = 10 ** (np.repeat(rng.uniform(-80, -20, n // 500 + 1), 500)[:n] / 20)
    return rand(rng, n, t) * level.astype(np.float32)


def carrier(rng, n, t):
    """tests/test_gpu_pll.py locked_signal: a carrier inside the loop's range, 20 dB of noise under it"""
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return (np.exp(1j * (2 * np.pi * 0.1 * np.arange(n) + 0.3)) + 0.1 * noise).astype(np.complex64)


def concat(obj, pieces):
    return np.concatenate([np.ravel(obj.process(p)) for p in pieces])


def welch_average(obj, pieces):
    for p in pieces:
        obj.process(p)
    return obj.average()


class _Welch(lr.spectrum_utils.WelchSpectrum):
    def reset(self):
        _lib.check(_lib.load().lrhip_stage_reset(self._stage), "welch:reset")


# ---- the bounds of the rows that are not byte-exact, each as the test it is taken from states it
def within_abs(eps):
    return lambda got, want: len(got) == len(want) and float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))) < eps


def agc_bound(got, want):
    """test_gpu_parity.py::test_agc_parallel_scans_vs_sequential_oracle"""
    return len(got) == len(want) and float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-6))) < 2e-5


def squelch_bound(got, want):
    """test_gpu_parity.py::test_golden_powersquelch_and_large: a threshold crossing may land one sample apart"""
    return len(got) == len(want) and np.count_nonzero(got != want) <= 2


def iir_bound(case):
    """test_gpu_iir_forms.py (tests/helpers/iir_forms.py bar): 10 * yard + 2e-6 * scale"""
    @functools.lru_cache(maxsize=None)
    def limit():
        _, _, yard, scale = F.reference(case)
        return F.bar(yard, scale)
    return lambda got, want: len(got) == len(want) and float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))) <= limit()


Row = collections.namedtuple("Row", "name create type n tile align seek bound source signal run form")


def row(name, create, type_, n, tile, align=1, seek=None, bound=None, source="", signal=rand, run=concat, form=None):
    """tile: the stage's tile in input samples; seek: an n0 for the stages with a seek() of their own; bound / source: the comparison of ragged
    against whole where it is not byte-exact, and the test it comes from (source alone: the test that states the exactness)"""
    assert n <= 1 << 16 and n > 2 * tile + 1
    return pytest.param(Row(name, create, type_, n, tile, align, seek, bound, source, signal, run, form), id=name)


def iir_row(name, form, cplx, P, r, nb, seed, **kw):
    n = 2 * F.TILE + 333
    case = F.make_case("carried", cplx, P, r, nb, seed, n=n, **kw)
    assert F.iir_form(case.b, case.a)[0] == form, (name, F.iir_form(case.b, case.a))
    t = C if cplx else R
    # (the three-pass form is left out of the exact comparison on tile-aligned cuts: a call's second tile starts from the carry scan's matrix
    # powers, a second call from the carried outputs themselves, and the two differ in the last bits - before the carried-state types as after)
    return row(name, lambda: make(lr.IIRFilterBlock, [case.b, case.a], t), t, n, F.TILE, align=F.TILE if form in ("oneshot", "stream") else 1, seek=3 * F.TILE,
               bound=iir_bound(case), source="test_gpu_iir_forms.py bar", signal=lambda rng, n_, t_: F.case_input(case))


def firwin_iir():
    """FIRFilterBlock(32 taps) -> FMDeemphasisFilterBlock as a chain: the fused register-window kernel (FirWinRealStage with its recurrence)"""
    taps = filter_utils.firwin_lowpass(32, 0.2)
    return lr.Chain([make(lr.FIRFilterBlock, [np.asarray(taps, np.float32), "auto"], R, rate=220500.0), make(lr.FMDeemphasisFilterBlock, [75e-6], R, rate=220500.0)])


def pll(knobs):
    blk = B.PLLOutBlock(0.01, 0.19, 0.21, 3.0, "out")
    blk.rate = 2.0
    blk.op_knobs = knobs
    blk.differentiate([C])
    blk.initialize()
    return lr.Chain([blk])


def viterbi(soft):
    return make(lr.ViterbiDecoderBlock, [3, [0o7, 0o5], {"soft": soft, "block": 64, "depth": 2}], R if soft else BIT)


def llrs(rng, n, t):
    return rng.standard_normal(n).astype(np.float32)


K3 = [3, [0o7, 0o5]]
ROWS = [
    row("fmdiscrim", lambda: make(lr.FrequencyDiscriminatorBlock, [1.25], C), C, 2 * 1024 + 333, 1024, bound=within_abs(1e-6),
        source="test_gpu_parity.py::test_discriminator_vs_oracle"),
    row("fmmod", lambda: make(lr.FrequencyModulatorBlock, [0.2], R), R, 2 * 4096 + 333, 4096,
        source="test_gpu_parity.py::test_frequencymodulator_large_exact_phase_any_chunking"),
    row("delay-scalar", lambda: make(lr.DelayBlock, [7], C), C, 2 * 256 + 77, 256, source="test_gpu_parity.py::test_golden_rank3_blocks"),
    row("delay-vec", lambda: make(lr.DelayBlock, [8], C), C, 2 * 512 + 78, 512, source="test_gpu_parity.py::test_golden_rank3_blocks"),
    row("diffdec", lambda: make(lr.DifferentialDecoderBlock, [], BIT), BIT, 2 * 256 + 77, 256, source="test_gpu_digital.py::test_golden_differentialdecoder"),
    iir_row("iir-single-launch-oneshot", "oneshot", False, 1, 0.5, 2, 9601),
    iir_row("iir-single-launch-stream", "stream", True, 1, 0.99, 2, 9602),
    iir_row("iir-three-pass", "threepass", False, 1, 0.9995, 2, 9603),
    iir_row("iir-three-pass-one-tap", "threepass", True, 1, 0.9995, 1, 9604),
    iir_row("iir-sequential", "seq", True, 9, 0.8, 3, 9605, lo=0.2, hi=2.9),
    row("agc", lambda: make(lr.AGCBlock, ["fast", -35, -60], C, rate=48000.0), C, 2 * 2048 + 333, 2048, bound=agc_bound,
        source="test_gpu_parity.py::test_agc_parallel_scans_vs_sequential_oracle", signal=levelled),
    row("squelch", lambda: make(lr.PowerSquelchBlock, [-45], C, rate=48000.0), C, 2 * 2048 + 333, 2048, bound=squelch_bound,
        source="test_gpu_parity.py::test_golden_powersquelch_and_large", signal=levelled),
    row("firwin+iir", firwin_iir, R, 2 * 4096 + 333, 4096, align=4096, seek=3 * 4096, bound=within_abs(5e-7),
        source="test_gpu_firwin.py::test_fir_iir_downsampler_fused_vs_oracle_and_unfused"),
    row("resample-interpolator", lambda: make(lr.InterpolatorBlock, [5], C), C, 2 * 1280 + 333, 1280, seek=1000,
        source="test_gpu_parity.py::test_polyphase_resampler_fusion_bit_equal_to_zero_stuffed_chain"),
    row("resample-rational", lambda: make(lr.RationalResamplerBlock, [3, 2], C), C, 2 * 1536 + 333, 1536, seek=1000,
        source="test_gpu_parity.py::test_polyphase_resampler_fusion_bit_equal_to_zero_stuffed_chain"),
    row("resample-generic", lambda: make(lr.RationalResamplerBlock, [7, 3], R), R, 2 * 110 + 33, 110, seek=100,
        source="test_gpu_parity.py::test_polyphase_resampler_fusion_bit_equal_to_zero_stuffed_chain"),
    row("channelizer-gemm", lambda: make(lr.PolyphaseChannelizerBlock, [32, filter_utils.firwin_lowpass(32, 1 / 32), {"method": "gemm"}], C), C,
        2 * 2048 + 333, 2048, source="test_gpu_channelizer.py::test_chunking_is_bit_invariant"),
    row("channelizer-fft", lambda: make(lr.PolyphaseChannelizerBlock, [8, filter_utils.firwin_lowpass(8, 1 / 8), {"method": "fft"}], C), C,
        2 * 2048 + 333, 2048, source="test_gpu_pfb_channelizer.py::test_chunking_is_bit_invariant"),
    row("channelizer-oversampled", lambda: make(lr.PolyphaseChannelizerBlock, [8, filter_utils.firwin_lowpass(8, 1 / 8), {"oversample": 2}], C), C,
        2 * 1024 + 333, 1024, source="test_gpu_pfb_oversampled.py::test_chunking_is_bit_invariant"),
    row("arbresampler", lambda: make(lr.ArbitraryResamplerBlock, [1.37, {"phases": 16, "taps_per_phase": 4}], C), C, 2 * 374 + 133, 374, seek=1000,
        source="test_gpu_arbresample.py::test_any_cut_of_the_stream_gives_the_same_bits"),
    row("welch", lambda: _Welch(C, 64, "hamming", 1e6, 0.5, 10.0), C, 2 * 64 * 64 + 333, 64 * 64, bound=within_abs(2e-3),
        source="test_gpu_parity.py::test_welch_spectrum_vs_oracle", run=welch_average),
    row("convenc", lambda: make(lr.ConvolutionalEncoderBlock, K3, BIT), BIT, 2 * 256 + 77, 256, seek=100,
        source="test_gpu_viterbi.py::test_encoder_history_across_calls_and_seek"),
    row("viterbi-soft", lambda: viterbi(True), R, 2 * 512 + 333, 512, seek=1000, source="test_gpu_viterbi.py::test_any_chunking_gives_the_same_bytes", signal=llrs),
    row("viterbi-hard", lambda: viterbi(False), BIT, 2 * 512 + 333, 512, seek=1000, source="test_gpu_viterbi.py::test_hard_input"),
    row("rsenc", lambda: make(lr.ReedSolomonEncoderBlock, [3, 1], BYTE), BYTE, 2 * 256 + 77, 256, seek=100,
        source="test_gpu_reedsolomon.py::test_any_chunking_gives_the_same_bytes"),
    row("rsdec", lambda: make(lr.ReedSolomonDecoderBlock, [3, 1], BYTE), BYTE, 2 * 768 + 77, 768, seek=100,
        source="test_gpu_reedsolomon.py::test_any_chunking_gives_the_same_bytes"),
    row("packbits", lambda: make(lr.PackBitsBlock, [], BIT), BIT, 2 * 2048 + 77, 2048, seek=100, source="test_gpu_reedsolomon.py::test_any_chunking_gives_the_same_bytes"),
    row("unpackbits", lambda: make(lr.UnpackBitsBlock, [], BYTE), BYTE, 2 * 256 + 77, 256, seek=100,
        source="test_gpu_reedsolomon.py::test_any_chunking_gives_the_same_bytes"),
    row("puncture", lambda: make(lr.PunctureBlock, ["110"], BIT), BIT, 2 * 768 + 77, 768, seek=100,
        source="test_gpu_fecglue.py::test_puncture_and_depuncture_against_the_model"),
    row("depuncture", lambda: make(lr.DepunctureBlock, ["110"], R), R, 2 * 512 + 77, 512, seek=100,
        source="test_gpu_fecglue.py::test_puncture_and_depuncture_against_the_model", signal=llrs),
    row("convinterleave", lambda: make(lr.ConvolutionalInterleaverBlock, [2, 1], BYTE), BYTE, 2 * 16384 + 333, 16384, seek=1001,
        source="test_gpu_fecglue.py::test_interleavers_against_the_model"),
    row("convdeinterleave", lambda: make(lr.ConvolutionalDeinterleaverBlock, [2, 1], BYTE), BYTE, 2 * 16384 + 333, 16384, seek=1001,
        source="test_gpu_fecglue.py::test_interleavers_against_the_model"),
    row("phasecorr", lambda: make(lr.BinaryPhaseCorrectorBlock, [4, 2], C), C, 2 * 4096 + 333, 4096, seek=1001,
        source="test_gpu_phasecorr.py::test_ragged_calls_bit_identical", signal=carrier),
    row("pll-serial", lambda: pll(":speculate=0"), C, 2 * 4096 + 333, 4096, bound=within_abs(1e-6), source="test_gpu_pll.py::test_serial_path",
        signal=carrier, form=(1,)),
    row("pll-speculative", lambda: pll(":segment=64"), C, 2 * 4096 + 333, 4096, bound=within_abs(1e-6),
        source="test_gpu_pll.py::test_locked_parity_whole_and_ragged", signal=carrier, form=(4, 5)),
    row("pam", lambda: make(lr.PulseAmplitudeModulatorBlock, [1.0, 3.0, 4, {"msb_first": True}], BIT), BIT, 2 * 2731 + 333, 2731, seek=1000,
        source="test_gpu_modulator.py::test_random_bits_ragged_chunks"),
    row("qam", lambda: make(lr.QuadratureAmplitudeModulatorBlock, [1.0, 1.0, 4, {"msb_first": False}], BIT), BIT, 2 * 4096 + 333, 4096, seek=1000,
        source="test_gpu_modulator.py::test_random_bits_ragged_chunks"),
]


def same_bytes(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


@functools.lru_cache(maxsize=None)
def whole(r):
    """(input, a fresh stage's output for it in one call), computed once per row and left alone"""
    x = r.signal(np.random.default_rng(len(r.name) * 1000 + r.n), r.n, r.type)
    obj = r.create()
    y = r.run(obj, [x])
    if r.form is not None:
        assert obj.last_launches in r.form, (r.name, obj.last_launches)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def pieces(x, cuts):
    edges = [0] + [c for c in cuts if c < len(x)] + [len(x)]
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("r", ROWS)
def test_reset_after_an_odd_number_of_calls(r):
    x, want = whole(r)
    obj = r.create()
    r.run(obj, pieces(x, [7, 7 + r.tile + 1]))               # three calls of unequal length: the pair sits on its second slot
    obj.reset()
    assert same_bytes(r.run(obj, [x]), want), r.name
    if r.seek is not None:
        r.run(obj, pieces(x, [5, 5 + r.tile + 2]))
        obj.seek(r.seek)
        fresh = r.create()
        fresh.seek(r.seek)
        assert same_bytes(r.run(obj, [x]), r.run(fresh, [x])), (r.name, r.seek)


@pytest.mark.parametrize("r", ROWS)
def test_ragged_calls_against_one_call(r):
    x, want = whole(r)
    got = r.run(r.create(), pieces(x, [1, 2, r.tile - 1, r.tile, r.tile + 1]))
    if r.bound is None:
        assert same_bytes(got, want), (r.name, r.source)
    else:
        assert r.bound(got, want), (r.name, r.source)
    if r.align > 1:
        assert same_bytes(r.run(r.create(), pieces(x, [r.align, 2 * r.align])), want), (r.name, "cuts on multiples of align()")
