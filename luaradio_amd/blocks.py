"""Device variants of the signal blocks on the hot path (same names, arguments and semantics as the
reference's radio/blocks/signal/*.lua).  All arithmetic runs in liblrhip.so on the GPU; this file is the
host glue the reference keeps in Lua (tap design, argument checks, rate bookkeeping).
"""
import math

import numpy as np

from . import _lib, filter_utils, types
from .block import Block, Input, Output, _fptr, as_taps, fir_mode


class FIRFilterBlock(Block):
    """radio/blocks/signal/firfilter.lua.  FIRFilterBlock(taps[, use_fft]).

    use_fft (block.fir_mode, the same table as the Lua glue's lrhip.fir_mode): True is the reference's overlap-save
    (firfilter.lua:320-398: only whole L = N-M+1 blocks are emitted, tail retained); "fast" runs the same overlap-save
    arithmetic (fused FFT kernel) but emits one output per input; None (the default, as `nil` in the reference, which then picks
    its FFT form when FFTW is present, firfilter.lua:57) and "auto" pick "fast" from 48 taps up and the direct form below; False
    is the direct form on the f32 matrix cores, bit-identical to the fmaf chain in the reference's tap order."""
    name = "FIRFilterBlock"

    def instantiate(self, taps, use_fft=None):
        self.taps = as_taps(taps)
        self.use_fft = fir_mode(use_fft)
        self.decimation = 1
        if self.taps.dtype == np.complex64:      # firfilter.lua:68-74
            self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        else:
            self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
            self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def initialize(self):
        L = _lib.load()
        tc = self.taps.dtype == np.complex64
        flat = self.taps.view(np.float32) if tc else self.taps
        self._set_stage(L.lrhip_fir_create(_fptr(flat), len(self.taps), int(tc),
                                           int(self.get_input_type() is types.ComplexFloat32),
                                           self.decimation, int(self.use_fft)),
                        "Creating lrhip fir object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class LowpassFilterBlock(FIRFilterBlock):
    """radio/blocks/signal/lowpassfilter.lua:32-50. LowpassFilterBlock(num_taps, cutoff[, nyquist[, window]])."""
    name = "LowpassFilterBlock"

    def instantiate(self, num_taps, cutoff, nyquist=None, window=None):
        assert num_taps, "Missing argument #1 (num_taps)"
        assert cutoff is not None, "Missing argument #2 (cutoff)"
        self.cutoff = cutoff
        self.window = window or "hamming"
        self.nyquist = nyquist
        FIRFilterBlock.instantiate(self, types.Float32.vector(num_taps))

    def _design(self, nyquist):
        return filter_utils.firwin_lowpass(len(self.taps), self.cutoff / nyquist, self.window)

    def initialize(self):
        nyquist = self.nyquist or (self.get_rate() / 2)       # lowpassfilter.lua:43
        self.taps = types.Float32.vector_from_array(self._design(nyquist))
        FIRFilterBlock.initialize(self)


class HighpassFilterBlock(LowpassFilterBlock):
    """radio/blocks/signal/highpassfilter.lua"""
    name = "HighpassFilterBlock"

    def _design(self, nyquist):
        return filter_utils.firwin_highpass(len(self.taps), self.cutoff / nyquist, self.window)


class BandpassFilterBlock(LowpassFilterBlock):
    """radio/blocks/signal/bandpassfilter.lua: cutoff = {low, high}"""
    name = "BandpassFilterBlock"

    def _design(self, nyquist):
        return filter_utils.firwin_bandpass(len(self.taps), [self.cutoff[0] / nyquist, self.cutoff[1] / nyquist], self.window)


class BandstopFilterBlock(LowpassFilterBlock):
    """radio/blocks/signal/bandstopfilter.lua: cutoff = {low, high}"""
    name = "BandstopFilterBlock"

    def _design(self, nyquist):
        return filter_utils.firwin_bandstop(len(self.taps), [self.cutoff[0] / nyquist, self.cutoff[1] / nyquist], self.window)


class FrequencyTranslatorBlock(Block):
    """radio/blocks/signal/frequencytranslator.lua:26-30, :93-110. FrequencyTranslatorBlock(offset)."""
    name = "FrequencyTranslatorBlock"

    def instantiate(self, offset):
        assert offset is not None, "Missing argument #1 (offset)"
        self.offset = offset
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])

    def initialize(self):
        self.omega = 2 * math.pi * (self.offset / self.get_rate())     # frequencytranslator.lua:95
        self._set_stage(_lib.load().lrhip_rotator_create(self.omega), "Creating lrhip rotator object")

    def process(self, x):
        return self._execute(x, np.complex64)


class DownsamplerBlock(Block):
    """radio/blocks/signal/downsampler.lua:29-56. DownsamplerBlock(factor)."""
    name = "DownsamplerBlock"

    def instantiate(self, factor):
        assert factor, "Missing argument #1 (factor)"
        self.factor = int(factor)
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def get_rate(self):
        return Block.get_rate(self) / self.factor          # downsampler.lua:36-38

    def initialize(self):
        self._set_stage(_lib.load().lrhip_downsampler_create(self.factor, self.get_input_type().size),
                        "Creating lrhip downsampler object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class FrequencyDiscriminatorBlock(Block):
    """radio/blocks/signal/frequencydiscriminator.lua:25-38. FrequencyDiscriminatorBlock(modulation_index)."""
    name = "FrequencyDiscriminatorBlock"

    def instantiate(self, modulation_index):
        assert modulation_index, "Missing argument #1 (modulation_index)"
        self.gain = 2 * math.pi * modulation_index          # frequencydiscriminator.lua:28
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.Float32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_fmdiscrim_create(self.gain), "Creating lrhip fmdiscrim object")

    def process(self, x):
        return self._execute(x, np.float32)


class IIRFilterBlock(Block):
    """radio/blocks/signal/iirfilter.lua:39-61. IIRFilterBlock(b_taps, a_taps)."""
    name = "IIRFilterBlock"

    def instantiate(self, b_taps, a_taps):
        assert b_taps is not None, "Missing argument #1 (b_taps)"
        assert a_taps is not None, "Missing argument #2 (a_taps)"
        self.b_taps = types.Float32.vector_from_array(b_taps)
        self.a_taps = types.Float32.vector_from_array(a_taps)
        assert len(self.a_taps) >= 1, "Feedback taps must be at least length 1"
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_iir_create(_fptr(self.b_taps), len(self.b_taps), _fptr(self.a_taps), len(self.a_taps),
                                                     int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip iir object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class SinglepoleLowpassFilterBlock(IIRFilterBlock):
    """radio/blocks/signal/singlepolelowpassfilter.lua:27-67. SinglepoleLowpassFilterBlock(cutoff)."""
    name = "SinglepoleLowpassFilterBlock"

    def instantiate(self, cutoff):
        assert cutoff, "Missing argument #1 (cutoff)"
        self.cutoff = cutoff
        IIRFilterBlock.instantiate(self, types.Float32.vector(2), types.Float32.vector(2))

    def initialize(self):
        rate = self.get_rate()
        tau = 1 / (2 * math.pi * self.cutoff)                       # :57
        tau = 1 / (2 * rate * math.tan(1 / (2 * rate * tau)))       # :58 pre-warp
        self.b_taps = types.Float32.vector_from_array([1 / (1 + 2 * tau * rate), 1 / (1 + 2 * tau * rate)])
        self.a_taps = types.Float32.vector_from_array([1, (1 - 2 * tau * rate) / (1 + 2 * tau * rate)])
        IIRFilterBlock.initialize(self)


class FMDeemphasisFilterBlock(SinglepoleLowpassFilterBlock):
    """radio/blocks/signal/fmdeemphasisfilter.lua:24-27. FMDeemphasisFilterBlock(tau)."""
    name = "FMDeemphasisFilterBlock"

    def instantiate(self, tau):
        assert tau, "Missing argument #1 (tau)"
        SinglepoleLowpassFilterBlock.instantiate(self, 1 / (2 * math.pi * tau))


class _BinaryBlock(Block):
    """Two-input element-wise blocks (MultiplyBlock, MultiplyConjugateBlock, AddBlock, SubtractBlock)."""
    _op = "multiply"
    _complex_only = False

    def instantiate(self):
        self.add_type_signature([Input("in1", types.ComplexFloat32), Input("in2", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        if not self._complex_only:
            self.add_type_signature([Input("in1", types.Float32), Input("in2", types.Float32)], [Output("out", types.Float32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_binary_create(self._op.encode(), int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip %s object" % self._op)

    def process(self, x, y):
        import ctypes as C
        L = _lib.load()
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        dt = self.get_input_type().dtype
        if x.dtype != dt or y.dtype != dt or len(x) != len(y):
            raise TypeError("Block %s expects two %s vectors of equal length" % (self.name, self.get_input_type()))
        out = np.empty(len(x), dtype=self.get_output_type().dtype)
        n = L.lrhip_stage_execute2(self._stage, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x),
                                   out.ctypes.data_as(C.c_void_p), len(out))
        _lib.check(n, "%s:process" % self.name)
        return out[:n]


class MultiplyBlock(_BinaryBlock):
    """radio/blocks/signal/multiply.lua"""
    name, _op = "MultiplyBlock", "multiply"


class MultiplyConjugateBlock(_BinaryBlock):
    """radio/blocks/signal/multiplyconjugate.lua"""
    name, _op, _complex_only = "MultiplyConjugateBlock", "multiplyconjugate", True


class AddBlock(_BinaryBlock):
    """radio/blocks/signal/add.lua"""
    name, _op = "AddBlock", "add"


class SubtractBlock(_BinaryBlock):
    """radio/blocks/signal/subtract.lua"""
    name, _op = "SubtractBlock", "subtract"


class ComplexBandpassFilterBlock(FIRFilterBlock):
    """radio/blocks/signal/complexbandpassfilter.lua. ComplexBandpassFilterBlock(num_taps, cutoffs[, nyquist[, window]])."""
    name = "ComplexBandpassFilterBlock"
    _design = staticmethod(filter_utils.firwin_complex_bandpass)

    def instantiate(self, num_taps, cutoffs, nyquist=None, window=None):
        assert num_taps, "Missing argument #1 (num_taps)"
        assert cutoffs is not None, "Missing argument #2 (cutoffs)"
        self.cutoffs, self.window, self.nyquist = cutoffs, window or "hamming", nyquist
        FIRFilterBlock.instantiate(self, types.ComplexFloat32.vector(num_taps))

    def initialize(self):
        nyquist = self.nyquist or (self.get_rate() / 2)
        taps = self._design(len(self.taps), [self.cutoffs[0] / nyquist, self.cutoffs[1] / nyquist], self.window)
        self.taps = types.ComplexFloat32.vector_from_array(taps)
        FIRFilterBlock.initialize(self)


class ComplexBandstopFilterBlock(ComplexBandpassFilterBlock):
    """radio/blocks/signal/complexbandstopfilter.lua"""
    name = "ComplexBandstopFilterBlock"
    _design = staticmethod(filter_utils.firwin_complex_bandstop)


class RootRaisedCosineFilterBlock(FIRFilterBlock):
    """radio/blocks/signal/rootraisedcosinefilter.lua. RootRaisedCosineFilterBlock(num_taps, beta, symbol_rate)."""
    name = "RootRaisedCosineFilterBlock"

    def instantiate(self, num_taps, beta, symbol_rate):
        assert num_taps, "Missing argument #1 (num_taps)"
        assert beta is not None, "Missing argument #2 (beta)"
        assert symbol_rate, "Missing argument #3 (symbol_rate)"
        self.beta, self.symbol_rate = beta, symbol_rate
        FIRFilterBlock.instantiate(self, types.Float32.vector(num_taps))

    def initialize(self):
        taps = filter_utils.fir_root_raised_cosine(len(self.taps), self.get_rate(), self.beta, 1 / self.symbol_rate)
        self.taps = types.Float32.vector_from_array(taps)
        FIRFilterBlock.initialize(self)


class MultiplyConstantBlock(Block):
    """radio/blocks/signal/multiplyconstant.lua. MultiplyConstantBlock(constant): number / Float32 or a complex constant."""
    name = "MultiplyConstantBlock"

    def instantiate(self, constant):
        assert constant is not None, "Missing argument #1 (constant)"
        if isinstance(constant, (complex, np.complexfloating)):
            self.constant = np.complex64(constant)
            self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        elif isinstance(constant, (int, float, np.floating, np.integer)):
            self.constant = np.float32(constant)
            self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])
            self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        else:
            raise TypeError("Unsupported constant type")

    def initialize(self):
        cc = isinstance(self.constant, np.complexfloating)
        self._set_stage(_lib.load().lrhip_multiply_constant_create(float(np.real(self.constant)), float(np.imag(self.constant)), int(cc),
                                                                   int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip multiplyconstant object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class UpsamplerBlock(Block):
    """radio/blocks/signal/upsampler.lua. UpsamplerBlock(factor)."""
    name = "UpsamplerBlock"

    def instantiate(self, factor):
        assert factor, "Missing argument #1 (factor)"
        self.factor = int(factor)
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def get_rate(self):
        return Block.get_rate(self) * self.factor          # upsampler.lua:41-43

    def initialize(self):
        self._set_stage(_lib.load().lrhip_upsampler_create(self.factor, self.get_input_type().size), "Creating lrhip upsampler object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class PolyphaseChannelizerBlock(Block):
    """Critically sampled K-channel analysis filterbank (BASELINE.json configs[4]).  Not a block of the reference: it is
    K parallel chains FrequencyTranslatorBlock(-c*rate/K) -> FIRFilterBlock(taps) -> DownsamplerBlock(K).
    PolyphaseChannelizerBlock(num_channels[, taps[, options]]); default prototype = firwin_lowpass(16*K, 1/K).
    Output: frames of K ComplexFloat32 (channel c at position c), one per K inputs.
    options = {"method": "gemm" | "fft"}: "gemm" is one dense GEMM on the f32 matrix cores (K in {32, 64}, len(taps) a multiple
    of 32 up to 8192), "fft" the polyphase + FFT form (K a power of two in [8, 4096], K <= len(taps) <= min(64 K, 65536)).
    Without a method: the GEMM where it accepts the shape, the FFT form otherwise.
    options["oversample"] = 2 or 4 (default 1): the hop is D = K / oversample, one frame per D inputs, each channel at oversample * rate / K,
    and frame m * oversample is frame m of the critically sampled bank.  The FFT form only."""
    name = "PolyphaseChannelizerBlock"

    def instantiate(self, num_channels, taps=None, options=None):
        assert num_channels, "Missing argument #1 (num_channels)"
        self.num_channels = int(num_channels)
        if taps is None:
            taps = filter_utils.firwin_lowpass(16 * self.num_channels, 1.0 / self.num_channels)
        self.taps = types.Float32.vector_from_array(taps)
        self.method = (options or {}).get("method")
        assert self.method in (None, "gemm", "fft"), "Unsupported method \"%s\" (\"gemm\" or \"fft\")" % self.method
        self.oversample = (options or {}).get("oversample", 1)
        assert self.oversample in (1, 2, 4), "Unsupported oversample \"%s\" (1, 2 or 4)" % (self.oversample,)
        if self.oversample > 1 and self.method == "gemm":
            raise ValueError("oversample = %d needs the FFT form: the GEMM (method = \"gemm\") is critically sampled only" % self.oversample)
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])

    def get_rate(self):
        return Block.get_rate(self) * self.oversample      # K values per K / oversample input samples; each channel runs at oversample * rate / K

    def gemm_accepts(self):
        """the domain of lrhip_channelizer_create"""
        return self.num_channels in (32, 64) and 32 <= len(self.taps) <= 8192 and len(self.taps) % 32 == 0

    def initialize(self):
        L = _lib.load()
        if self.oversample > 1:
            self._set_stage(L.lrhip_pfb_oversampled_create(_fptr(self.taps), len(self.taps), self.num_channels, self.oversample),
                            "Creating lrhip oversampled channelizer object")
            return
        fft = self.method == "fft" or (self.method is None and not self.gemm_accepts())
        create = L.lrhip_pfb_channelizer_create if fft else L.lrhip_channelizer_create
        self._set_stage(create(_fptr(self.taps), len(self.taps), self.num_channels), "Creating lrhip channelizer object")

    def process(self, x):
        """returns an array of shape (frames, K)"""
        return self._execute(x, np.complex64).reshape(-1, self.num_channels)


class PolyphaseSynthesizerBlock(Block):
    """K-channel synthesis filterbank in its polyphase + FFT form, the inverse of PolyphaseChannelizerBlock.  Not a block of the reference: it is
    K parallel chains UpsamplerBlock(D) -> FIRFilterBlock(taps) -> FrequencyTranslatorBlock(+c*rate_out/K), c = 0 .. K-1, summed, D = K / oversample.
    PolyphaseSynthesizerBlock(num_channels[, taps[, options]]); default prototype = firwin_lowpass(16*K, 1/K).
    Input: the frame stream the analysis bank emits, K ComplexFloat32 values per frame (channel c at position c); a call may end inside a frame,
    whose values wait for the next call.  Output: D samples per completed frame.
    K a power of two in [8, 4096], K <= len(taps) <= min(64 K, 65536).  options["oversample"] = 2 or 4 (default 1): the frames come at hop D = K / oversample,
    as those of PolyphaseChannelizerBlock with the same option do; with a matched prototype on both sides the pair reconstructs its input."""
    name = "PolyphaseSynthesizerBlock"

    def instantiate(self, num_channels, taps=None, options=None):
        assert num_channels, "Missing argument #1 (num_channels)"
        self.num_channels = int(num_channels)
        if taps is None:
            taps = filter_utils.firwin_lowpass(16 * self.num_channels, 1.0 / self.num_channels)
        self.taps = types.Float32.vector_from_array(taps)
        self.oversample = (options or {}).get("oversample", 1)
        assert self.oversample in (1, 2, 4), "Unsupported oversample \"%s\" (1, 2 or 4)" % (self.oversample,)
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])

    def get_rate(self):
        return Block.get_rate(self) / self.oversample      # K values in per K / oversample samples out

    def op(self):
        """the stage as lrhip_unary_create takes it; %.9g gives every Float32 tap back exactly"""
        return "pfbsynthesizer:channels=%d:oversample=%d:taps=%s" % (self.num_channels, self.oversample,
                                                                     ",".join("%.9g" % float(v) for v in np.asarray(self.taps, np.float32)))

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 1), "Creating lrhip synthesizer object")

    def process(self, y):
        """y: an array of shape (frames, K) or the flat frame stream; returns the flat output stream"""
        return self._execute(np.ascontiguousarray(y).reshape(-1), np.complex64)


class ArbitraryResamplerBlock(Block):
    """Resampler for any rate ratio in [1/16, 16]: a polyphase bank of P phases, linearly interpolated between neighbouring phases (GNU Radio's
    pfb_arb_resampler, liquid-dsp's resamp).  Not a block of the reference, whose RationalResamplerBlock(L, D) spreads one 128-tap lowpass over L phases.
    ArbitraryResamplerBlock(ratio[, options]), ratio = output rate / input rate; ComplexFloat32 or Float32.
    options = {"phases": P, a power of two 16 .. 256 (64); "taps_per_phase": T0, even, 4 .. 32 (16); "taps": a prototype of exactly P * T Float32 values}
    with T = 2 * ceil(T0 / (2 * min(1, ratio))) taps per phase - the filter is stretched when decimating - and P * T <= 8192.
    The default prototype is P * firwin_lowpass(P * T, min(1, ratio) / P).  The position of output m is m * step in 16.48 fixed point,
    step = rint(2^48 / ratio): the ratio in effect is effective_ratio = 2^48 / step, and the output is bit-identical however the stream is cut
    (luaradio_amd/csrc/kernels_arbresample.h has the arithmetic).  A call returns the outputs whose newest input has arrived, possibly none."""
    name = "ArbitraryResamplerBlock"

    @staticmethod
    def taps_per_phase(ratio, t0=16):
        """T: T0 stretched by the decimation, kept even"""
        return 2 * math.ceil(t0 / (2 * min(1.0, ratio)))

    def instantiate(self, ratio, options=None):
        assert ratio is not None, "Missing argument #1 (ratio)"
        options = options or {}
        ratio = float(ratio)
        if not (math.isfinite(ratio) and 1 / 16 <= ratio <= 16):
            raise ValueError("arbresampler: ratio must be a finite number in [1/16, 16], got %r" % ratio)
        self.phases = options.get("phases", 64)
        if self.phases not in (16, 32, 64, 128, 256):
            raise ValueError("arbresampler: phases must be a power of two in [16, 256], got %r" % (self.phases,))
        t0 = options.get("taps_per_phase", 16)
        if not (isinstance(t0, (int, np.integer)) and 4 <= t0 <= 32 and t0 % 2 == 0):
            raise ValueError("arbresampler: taps_per_phase must be an even integer in [4, 32], got %r" % (t0,))
        self.ratio = ratio
        self.num_taps = self.taps_per_phase(ratio, int(t0))
        P, T = self.phases, self.num_taps
        if P * T > 8192:
            raise ValueError("arbresampler: phases * taps per phase must not exceed 8192 (got phases = %d with %d taps per phase at ratio %r): "
                             "use fewer phases" % (P, T, ratio))
        self.step = int(np.rint(2.0 ** 48 / ratio))
        self.effective_ratio = 2.0 ** 48 / self.step
        taps = options.get("taps")
        if taps is None:
            # RationalResamplerBlock's convention, gain P: designed in double, rounded once to Float32
            taps = P * np.asarray(filter_utils.firwin_lowpass(P * T, min(1.0, ratio) / P), np.float64)
        self.taps = types.Float32.vector_from_array(taps)
        if len(self.taps) != P * T:
            raise ValueError("arbresampler: taps must hold exactly phases * taps per phase = %d * %d values, got %d" % (P, T, len(self.taps)))
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def get_rate(self):
        return Block.get_rate(self) * self.effective_ratio

    def op(self):
        """the stage as lrhip_unary_create takes it; %.9g gives every Float32 tap back exactly"""
        return "arbresampler:type=%s:phases=%d:step=%d:taps=%s" % ("cf32" if self.get_input_type() is types.ComplexFloat32 else "f32", self.phases, self.step,
                                                                  ",".join("%.9g" % float(v) for v in np.asarray(self.taps, np.float32)))

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip arbresampler object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class _UnaryBlock(Block):
    """One-input element-wise blocks with fixed types."""
    _op, _in, _out = "", types.ComplexFloat32, types.Float32

    def instantiate(self):
        self.add_type_signature([Input("in", self._in)], [Output("out", self._out)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self._op.encode(), 0.0, 0.0, 0, int(self._in is types.ComplexFloat32)),
                        "Creating lrhip %s object" % self._op)

    def process(self, x):
        return self._execute(x, self._out.dtype)


class ComplexMagnitudeBlock(_UnaryBlock):
    """radio/blocks/signal/complexmagnitude.lua"""
    name, _op = "ComplexMagnitudeBlock", "complexmagnitude"


class ComplexPhaseBlock(_UnaryBlock):
    """radio/blocks/signal/complexphase.lua"""
    name, _op = "ComplexPhaseBlock", "complexphase"


class ComplexToRealBlock(_UnaryBlock):
    """radio/blocks/signal/complextoreal.lua"""
    name, _op = "ComplexToRealBlock", "complextoreal"


class ComplexToImagBlock(_UnaryBlock):
    """radio/blocks/signal/complextoimag.lua"""
    name, _op = "ComplexToImagBlock", "complextoimag"


class ComplexConjugateBlock(_UnaryBlock):
    """radio/blocks/signal/complexconjugate.lua"""
    name, _op, _out = "ComplexConjugateBlock", "complexconjugate", types.ComplexFloat32


class RealToComplexBlock(_UnaryBlock):
    """radio/blocks/signal/realtocomplex.lua"""
    name, _op, _in, _out = "RealToComplexBlock", "realtocomplex", types.Float32, types.ComplexFloat32


class AbsoluteValueBlock(_UnaryBlock):
    """radio/blocks/signal/absolutevalue.lua"""
    name, _op, _in, _out = "AbsoluteValueBlock", "absolutevalue", types.Float32, types.Float32


class AddConstantBlock(MultiplyConstantBlock):
    """radio/blocks/signal/addconstant.lua. AddConstantBlock(constant)."""
    name = "AddConstantBlock"

    def initialize(self):
        cc = isinstance(self.constant, np.complexfloating)
        self._set_stage(_lib.load().lrhip_unary_create(b"addconstant", float(np.real(self.constant)), float(np.imag(self.constant)), int(cc),
                                                       int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip addconstant object")


class DelayBlock(Block):
    """radio/blocks/signal/delay.lua. DelayBlock(num_samples) (ComplexFloat32 / Float32 signatures)."""
    name = "DelayBlock"

    def instantiate(self, num_samples):
        assert num_samples is not None, "Missing argument #1 (num_samples)"
        assert num_samples > 0, "Number of samples must be greater than 0"
        self.num_samples = int(num_samples)
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_delay_create(self.num_samples, self.get_input_type().size), "Creating lrhip delay object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class HilbertTransformBlock(Block):
    """radio/blocks/signal/hilberttransform.lua. HilbertTransformBlock(num_taps[, window]): Float32 -> ComplexFloat32."""
    name = "HilbertTransformBlock"

    def instantiate(self, num_taps, window=None):
        assert num_taps, "Missing argument #1 (num_taps)"
        assert (num_taps % 2) == 1, "Number of taps must be odd"
        self.hilbert_taps = types.Float32.vector_from_array(filter_utils.fir_hilbert_transform(num_taps, window or "hamming"))
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.ComplexFloat32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_hilbert_create(_fptr(self.hilbert_taps), len(self.hilbert_taps)), "Creating lrhip hilbert object")

    def process(self, x):
        return self._execute(x, np.complex64)


class SinglepoleHighpassFilterBlock(IIRFilterBlock):
    """radio/blocks/signal/singlepolehighpassfilter.lua:27-48. SinglepoleHighpassFilterBlock(cutoff)."""
    name = "SinglepoleHighpassFilterBlock"

    def instantiate(self, cutoff):
        assert cutoff is not None, "Missing argument #1 (cutoff)"
        self.cutoff = cutoff
        super().instantiate(types.Float32.vector(2), types.Float32.vector(2))

    def initialize(self):
        rate = self.get_rate()
        tau = 1 / (2 * math.pi * self.cutoff)                       # :36-37 warped time constant
        tau = 1 / (2 * rate * math.tan(1 / (2 * rate * tau)))
        self.b_taps[0] = (2 * tau * rate) / (1 + 2 * tau * rate)
        self.b_taps[1] = -(2 * tau * rate) / (1 + 2 * tau * rate)
        self.a_taps[0] = 1
        self.a_taps[1] = (1 - 2 * tau * rate) / (1 + 2 * tau * rate)
        super().initialize()


class FMPreemphasisFilterBlock(SinglepoleHighpassFilterBlock):
    """radio/blocks/signal/fmpreemphasisfilter.lua:30-33. FMPreemphasisFilterBlock(tau)."""
    name = "FMPreemphasisFilterBlock"

    def instantiate(self, tau):
        assert tau is not None, "Missing argument #1 (tau)"
        super().instantiate(1 / (2 * math.pi * tau))


class FloatToComplexBlock(_BinaryBlock):
    """radio/blocks/signal/floattocomplex.lua: (real, imag) Float32 inputs -> ComplexFloat32."""
    name, _op = "FloatToComplexBlock", "floattocomplex"

    def instantiate(self):
        self.add_type_signature([Input("real", types.Float32), Input("imag", types.Float32)], [Output("out", types.ComplexFloat32)])


class ComplexToFloatBlock(Block):
    """radio/blocks/signal/complextofloat.lua: ComplexFloat32 -> (real, imag) Float32 outputs (two device passes)."""
    name = "ComplexToFloatBlock"

    def instantiate(self):
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("real", types.Float32), Output("imag", types.Float32)])

    def initialize(self):
        self._real, self._imag = ComplexToRealBlock(), ComplexToImagBlock()
        self._sub_blocks = [self._real, self._imag]       # DeviceGraph: one device pass per output
        for b in (self._real, self._imag):
            b.differentiate([types.ComplexFloat32])
            b.initialize()

    def process(self, x):
        return self._real.process(x), self._imag.process(x)


class FrequencyModulatorBlock(Block):
    """radio/blocks/signal/frequencymodulator.lua. FrequencyModulatorBlock(modulation_index): Float32 -> ComplexFloat32."""
    name = "FrequencyModulatorBlock"

    def instantiate(self, modulation_index):
        assert modulation_index is not None, "Missing argument #1 (modulation_index)"
        self.modulation_index = modulation_index
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.ComplexFloat32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_fmmod_create(float(self.modulation_index)), "Creating lrhip fmmod object")

    def process(self, x):
        return self._execute(x, np.complex64)


class PulseMatchedFilterBlock(FIRFilterBlock):
    """radio/blocks/signal/pulsematchedfilter.lua:27-47. PulseMatchedFilterBlock(baudrate[, invert=false])."""
    name = "PulseMatchedFilterBlock"
    _pattern = (1,)

    def instantiate(self, baudrate, invert=False):
        assert baudrate is not None, "Missing argument #1 (baudrate)"
        self.baudrate, self.invert = baudrate, bool(invert)
        FIRFilterBlock.instantiate(self, types.Float32.vector(32))

    def initialize(self):
        symbol_period = self.get_rate() / self.baudrate
        count = int(math.floor(symbol_period))            # Lua: for i = 1, symbol_period
        sign = -1.0 if self.invert else 1.0
        taps = []
        for half in self._pattern:
            taps.extend([sign * half] * count)
        self.taps = types.Float32.vector_from_array(taps)
        FIRFilterBlock.initialize(self)


class ManchesterMatchedFilterBlock(PulseMatchedFilterBlock):
    """radio/blocks/signal/manchestermatchedfilter.lua:27-50: a -1 half symbol followed by a +1 half symbol."""
    name = "ManchesterMatchedFilterBlock"
    _pattern = (-1, 1)


class AGCBlock(Block):
    """radio/blocks/signal/agc.lua:25-96. AGCBlock(mode[, target=-35[, threshold=-75[, {gain_tau=, power_tau=}]]])."""
    name = "AGCBlock"

    def instantiate(self, mode, target=None, threshold=None, options=None):
        assert mode, 'Missing argument #1 (mode), can be "fast", "slow", or "custom"'
        assert mode in ("fast", "slow", "custom"), 'Invalid mode "%s"' % mode
        options = options or {}
        self.mode = mode
        self.target = -35 if target is None else target
        self.threshold = -75 if threshold is None else threshold
        self.gain_tau = {"fast": 0.1, "slow": 3.0}.get(mode, options.get("gain_tau"))
        self.power_tau = options.get("power_tau") or 1.0
        assert self.gain_tau, 'Missing gain_tau parameter for "custom" mode'
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])

    def initialize(self):
        rate = self.get_rate()
        self._set_stage(_lib.load().lrhip_agc_create(1 / (1 + self.power_tau * rate), 1 / (1 + self.gain_tau * rate), 10 ** (self.target / 10),
                                                     10 ** (self.threshold / 10), int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip agc object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class PowerSquelchBlock(Block):
    """radio/blocks/signal/powersquelch.lua:26-80. PowerSquelchBlock(threshold_dBFS[, tau=0.001])."""
    name = "PowerSquelchBlock"

    def instantiate(self, threshold, tau=None):
        assert threshold is not None, "Missing argument #1 (threshold)"
        self.threshold = threshold
        self.tau = 0.001        # powersquelch.lua:28: `self.tau = tau or 0.001` reads an undefined global, so it is always 0.001
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_powersquelch_create(1 / (1 + self.tau * self.get_rate()), 10 ** (self.threshold / 10),
                                                              int(self.get_input_type() is types.ComplexFloat32)),
                        "Creating lrhip powersquelch object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


# ---- between a filtered baseband and a bit stream (luaradio_amd/csrc/stage_digital.h).  Double parameters travel in the op string as
# "name:key=value", each value as repr(float), which round-trips every double.
def digital_op(name, **params):
    return ":".join([name] + ["%s=%s" % (k, repr(float(v))) for k, v in params.items()])


class ZeroCrossingClockRecoveryBlock(Block):
    """radio/blocks/signal/zerocrossingclockrecovery.lua. ZeroCrossingClockRecoveryBlock(baudrate[, threshold=0.0]): Float32 -> +-1 clock."""
    name = "ZeroCrossingClockRecoveryBlock"

    def instantiate(self, baudrate, threshold=0.0):
        assert baudrate is not None, "Missing argument #1 (baudrate)"
        self.baudrate, self.threshold = baudrate, threshold
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def op(self):
        return digital_op("zerocrossingclockrecovery", period=self.get_rate() / self.baudrate, threshold=self.threshold)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip zerocrossingclockrecovery object")

    def process(self, x):
        return self._execute(x, np.float32)


class SamplerBlock(Block):
    """radio/blocks/signal/sampler.lua. SamplerBlock(): data (ComplexFloat32 or Float32) and a Float32 clock -> data where the clock rises.
    The output count depends on the clock."""
    name = "SamplerBlock"

    def instantiate(self):
        self.add_type_signature([Input("data", types.ComplexFloat32), Input("clock", types.Float32)], [Output("out", types.ComplexFloat32)])
        self.add_type_signature([Input("data", types.Float32), Input("clock", types.Float32)], [Output("out", types.Float32)])

    def initialize(self):
        self._set_stage(_lib.load().lrhip_binary_create(b"sampler", int(self.get_input_type() is types.ComplexFloat32)), "Creating lrhip sampler object")

    def process(self, data, clock):
        import ctypes as C
        L = _lib.load()
        data, clock = np.ascontiguousarray(data), np.ascontiguousarray(clock)
        if data.dtype != self.get_input_type().dtype or clock.dtype != np.float32 or len(data) != len(clock):
            raise TypeError("Block %s expects %s data and a Float32 clock of equal length" % (self.name, self.get_input_type()))
        cap = L.lrhip_stage_max_output(self._stage, len(data))
        out = np.empty(cap, dtype=self.get_output_type().dtype)
        n = L.lrhip_stage_execute2(self._stage, data.ctypes.data_as(C.c_void_p), clock.ctypes.data_as(C.c_void_p), len(data),
                                   out.ctypes.data_as(C.c_void_p), cap)
        _lib.check(n, "%s:process" % self.name)
        return out[:n]


class SlicerBlock(Block):
    """radio/blocks/signal/slicer.lua. SlicerBlock([threshold=0.0]): Float32 -> Bit, x > threshold."""
    name = "SlicerBlock"

    def instantiate(self, threshold=0.0):
        self.threshold = threshold
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Bit)])

    def op(self):
        return digital_op("slicer", threshold=self.threshold)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip slicer object")

    def process(self, x):
        return self._execute(x, np.uint8)


class DifferentialDecoderBlock(Block):
    """radio/blocks/signal/differentialdecoder.lua. DifferentialDecoderBlock([invert=false]): Bit -> Bit."""
    name = "DifferentialDecoderBlock"

    def instantiate(self, invert=False):
        self.invert = bool(invert)
        self.add_type_signature([Input("in", types.Bit)], [Output("out", types.Bit)])

    def op(self):
        return "differentialdecoder:invert=%d" % int(self.invert)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip differentialdecoder object")

    def process(self, x):
        return self._execute(x, np.uint8)


class ClockSamplerBlock(Block):
    """SamplerBlock(data = x, clock = ZeroCrossingClockRecoveryBlock(baudrate, threshold)(x)) as one one-input stage ("clocksampler"): the
    subgraph both the AX.25 and the POCSAG receivers use, without the +-1 clock stream.  Float32 -> Float32, data-dependent count.  A
    SlicerBlock (and a DifferentialDecoderBlock) right after it in a Chain run in its final pass."""
    name = "ClockSamplerBlock"

    def instantiate(self, baudrate, threshold=0.0):
        assert baudrate is not None, "Missing argument #1 (baudrate)"
        self.baudrate, self.threshold = baudrate, threshold
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def op(self):
        return digital_op("clocksampler", period=self.get_rate() / self.baudrate, threshold=self.threshold)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip clocksampler object")

    def process(self, x):
        return self._execute(x, np.float32)


class BinaryPhaseCorrectorBlock(Block):
    """radio/blocks/signal/binaryphasecorrector.lua. BinaryPhaseCorrectorBlock(num_samples[, sample_interval=32]): ComplexFloat32 ->
    ComplexFloat32, each sample rotated by minus the mean phase of the last num_samples measurements (one every sample_interval samples,
    clamped to [-pi/2, pi/2]).  A ComplexToRealBlock right after it in a Chain runs in its rotation pass."""
    name = "BinaryPhaseCorrectorBlock"

    def instantiate(self, num_samples, sample_interval=32):
        assert num_samples is not None, "Missing argument #1 (num_samples)"
        self.num_samples, self.sample_interval = num_samples, sample_interval
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32)])

    def op(self):
        return digital_op("binaryphasecorrector", num_samples=self.num_samples, sample_interval=self.sample_interval)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 1), "Creating lrhip binaryphasecorrector object")

    def process(self, x):
        return self._execute(x, np.complex64)


# ---- carrier recovery (luaradio_amd/csrc/stage_pll.h)
def pll_coefficients(loop_bandwidth, frequency_min, frequency_max, rate):
    """PLLBlock:initialize (pll.lua:117-126) in its operation order: (alpha, beta, freq_min, freq_max), frequencies in radians per sample."""
    loop_bw = 2 * math.pi * (loop_bandwidth / rate)
    freq_min = 2 * math.pi * (frequency_min / rate)
    freq_max = 2 * math.pi * (frequency_max / rate)
    damping = math.sqrt(2) / 2
    loop_bw = loop_bw / (damping + 1 / (4 * damping))
    denom = (1 + 2 * damping * loop_bw + loop_bw * loop_bw)
    alpha = (4 * damping * loop_bw) / denom
    beta = (4 * loop_bw * loop_bw) / denom
    return alpha, beta, freq_min, freq_max


class PLLOutBlock(Block):
    """One output port of PLLBlock as a one-output block: "out" (ComplexFloat32, cis(phi_multiplied)) or "error" (Float32).  The receivers that
    use the PLL's `out` alone take this block, so the loop runs once per call."""
    name = "PLLBlock"
    op_knobs = ""       # further "key=value" text for the op string (stage_pll.h: ":segment=64", ":warmup=8", ":speculate=0"), for tests and tools

    def instantiate(self, loop_bandwidth=None, frequency_min=None, frequency_max=None, multiplier=1.0, port="out"):
        assert loop_bandwidth is not None, "Missing argument #1 (loop_bandwidth)"
        assert frequency_min is not None, "Missing argument #2 (frequency_min)"
        assert frequency_max is not None, "Missing argument #3 (frequency_max)"
        assert port in ("out", "error"), 'port should be "out" or "error"'
        self.loop_bandwidth, self.frequency_min, self.frequency_max = loop_bandwidth, frequency_min, frequency_max
        self.multiplier = 1.0 if multiplier is None else multiplier
        self.port = port
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output(port, types.ComplexFloat32 if port == "out" else types.Float32)])

    def op(self):
        alpha, beta, freq_min, freq_max = pll_coefficients(self.loop_bandwidth, self.frequency_min, self.frequency_max, self.get_rate())
        return digital_op("pll", alpha=alpha, beta=beta, fmin=freq_min, fmax=freq_max, mult=self.multiplier) + ":port=" + self.port + self.op_knobs

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 1), "Creating lrhip pll object")

    def process(self, x):
        return self._execute(x, self.get_output_type().dtype)


class PLLBlock(Block):
    """radio/blocks/signal/pll.lua. PLLBlock(loop_bandwidth, frequency_min, frequency_max[, multiplier=1.0]): ComplexFloat32 -> out
    (ComplexFloat32, the locked oscillator at `multiplier` times the input's phase) and error (Float32, the phase detector).  One stage per
    port: the loop is deterministic, so both run the same trajectory from the same state.  Parallel in time while the loop is in lock
    (luaradio_amd/csrc/pll_plan.h: the contract); process(x) returns (out, error)."""
    name = "PLLBlock"
    op_knobs = ""       # as PLLOutBlock.op_knobs, handed to both ports' stages

    def instantiate(self, loop_bandwidth=None, frequency_min=None, frequency_max=None, multiplier=1.0):
        assert loop_bandwidth is not None, "Missing argument #1 (loop_bandwidth)"
        assert frequency_min is not None, "Missing argument #2 (frequency_min)"
        assert frequency_max is not None, "Missing argument #3 (frequency_max)"
        self.loop_bandwidth, self.frequency_min, self.frequency_max = loop_bandwidth, frequency_min, frequency_max
        self.multiplier = 1.0 if multiplier is None else multiplier
        self.add_type_signature([Input("in", types.ComplexFloat32)], [Output("out", types.ComplexFloat32), Output("error", types.Float32)])

    def initialize(self):
        self._out, self._error = (PLLOutBlock(self.loop_bandwidth, self.frequency_min, self.frequency_max, self.multiplier, port) for port in ("out", "error"))
        self._sub_blocks = [self._out, self._error]       # DeviceGraph: one device pass per output
        for b in self._sub_blocks:
            b.rate = self.get_rate()
            b.op_knobs = self.op_knobs
            b.differentiate([types.ComplexFloat32])
            b.initialize()

    def process(self, x):
        return self._out.process(x), self._error.process(x)

    def reset(self):
        for b in self._sub_blocks:
            b.reset()


# ---- the ERT receiver's blocks (luaradio_amd/csrc/stage_preamble.h)
PREAMBLE_SAMPLER_MAX_BUFFER = 1 << 21       # PS_MAX_B: the largest circular buffer 2^ceil_log2(period * #preamble + 1) the library accepts


def preamble_bits(preamble):
    """a Bit vector / any sequence of 0 / 1 -> list of ints; anything else is refused (preamblesampler.lua:43-44)"""
    if preamble is None:
        raise AssertionError("Missing argument #2 (preamble)")
    if isinstance(preamble, (str, bytes)) or not hasattr(preamble, "__len__"):
        raise TypeError("Unsupported data type for argument #2 (preamble), must be a Bit vector")
    bits = [v for v in (preamble.tolist() if isinstance(preamble, np.ndarray) else list(preamble))]
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v not in (0, 1) for v in bits):
        raise TypeError("Unsupported data type for argument #2 (preamble), must be a Bit vector (0 / 1 values)")
    return [int(v) for v in bits]


def preamble_sampler_params(rate, baudrate, preamble, num_samples):
    """(T, L, N, B) of a PreambleSamplerBlock at `rate`, with the library's create-time refusals (stage_preamble.h preamblesampler_create)"""
    bits = preamble_bits(preamble)
    T = int(math.floor(rate / baudrate))                 # preamblesampler.lua:50
    if T < 2:
        raise ValueError("preamblesampler: period must be >= 2 samples per symbol (got %d)" % T)
    if int(num_samples) != num_samples or num_samples < 2:
        raise ValueError("preamblesampler: num_samples must be an integer >= 2 (got %r)" % (num_samples,))
    if not bits:
        raise ValueError("preamblesampler: the preamble is empty")
    B = 1
    while B < T * len(bits) + 1:                         # 2^ceil_log2(T L + 1), preamblesampler.lua:52
        B *= 2
    if B > PREAMBLE_SAMPLER_MAX_BUFFER:
        raise ValueError("preamblesampler: period * preamble length = %d needs a buffer above the limit of %d samples"
                         % (T * len(bits), PREAMBLE_SAMPLER_MAX_BUFFER))
    return T, len(bits), int(num_samples), B


class PreambleSamplerBlock(Block):
    """radio/blocks/signal/preamblesampler.lua. PreambleSamplerBlock(baudrate, preamble, num_samples): Float32 -> Float32.  Finds the
    preamble (a Bit vector) at one tap per symbol, moves on while the preamble's energy does not degrade, then emits num_samples samples one
    symbol apart.  The output count depends on the data."""
    name = "PreambleSamplerBlock"

    def instantiate(self, baudrate, preamble, num_samples):
        assert baudrate is not None, "Missing argument #1 (baudrate)"
        assert preamble is not None, "Missing argument #2 (preamble)"
        assert num_samples is not None, "Missing argument #3 (frame length)"
        self.baudrate, self.preamble, self.num_samples = baudrate, preamble_bits(preamble), num_samples
        self.add_type_signature([Input("in", types.Float32)], [Output("out", types.Float32)])

    def op(self):
        T, _, N, _ = preamble_sampler_params(self.get_rate(), self.baudrate, self.preamble, self.num_samples)
        return "preamblesampler:period=%d:num_samples=%d:preamble=%s" % (T, N, "".join(map(str, self.preamble)))

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip preamblesampler object")

    def process(self, x):
        return self._execute(x, np.float32)


class ManchesterDecoderBlock(Block):
    """radio/blocks/signal/manchesterdecoder.lua. ManchesterDecoderBlock([invert=false]): Bit -> Bit, one output per 0,1 (0) or 1,0 (1) pair;
    an equal pair is a clock slip and the newer bit stays pending.  The output count depends on the data."""
    name = "ManchesterDecoderBlock"

    def instantiate(self, invert=False):
        self.invert = bool(invert)
        self.add_type_signature([Input("in", types.Bit)], [Output("out", types.Bit)])

    def op(self):
        return "manchesterdecoder:invert=%d" % int(self.invert)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip manchesterdecoder object")

    def process(self, x):
        return self._execute(x, np.uint8)


class VaricodeDecoderBlock(Block):
    """radio/blocks/protocol/varicodedecoder.lua. VaricodeDecoderBlock(): Bit -> Byte, the characters of a PSK31 bit stream: the bits in front of
    every 00 are looked up in the Varicode alphabet, and a state of more than 10 bits is dropped.  As in the reference the codes of 10 bits
    (`Z`, `?` and 38 more) are therefore never decoded, and a 9-bit code right behind one is lost with it.  The output count depends on the
    data and not on how the stream is cut into calls; process(x) returns a uint8 array, so bytes(y) is the text."""
    name = "VaricodeDecoderBlock"

    def instantiate(self):
        self.add_type_signature([Input("in", types.Bit)], [Output("out", types.Byte)])

    def op(self):
        return "varicodedecoder"

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip varicodedecoder object")

    def process(self, x):
        return self._execute(x, np.uint8)


class RDSFramerBlock(Block):
    """radio/blocks/protocol/rdsframer.lua. RDSFramerBlock(): Bit -> RDSFrameType, one record of four 16-bit data words per 104-bit window whose
    four blocks check (single-bit errors corrected); after a frame the search resumes behind it.  The output count depends on the data;
    process(x) returns an (n, 4) uint16 array."""
    name = "RDSFramerBlock"

    def instantiate(self):
        self.add_type_signature([Input("in", types.Bit)], [Output("out", types.RDSFrameType)])

    def op(self):
        return "rdsframer"

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip rdsframer object")

    def process(self, x):
        return self._execute(x, types.RDSFrameType.dtype)


class _ERTFramerBlock(Block):
    """The three ERT framers (luaradio_amd/csrc/stage_framers.h): Bit -> one structured record per frame.  They follow the reference's
    process() loops literally, the single-bit correction made inside the shift buffer included: a window that corrects a bit and then fails a
    later check leaves the flip behind for the windows after it.  The output count depends on the data; process(x) returns a structured array
    of the block's frame type, whose fields carry the reference's names."""
    _op = _frame_type = None

    def instantiate(self):
        self.add_type_signature([Input("in", types.Bit)], [Output("out", self._frame_type)])

    def op(self):
        return self._op

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % self._op)

    def process(self, x):
        return self._execute(x, self._frame_type.dtype)


class SCMFramerBlock(_ERTFramerBlock):
    """radio/blocks/protocol/scmframer.lua. SCMFramerBlock(): Bit -> SCMFrameType, one 16-byte record per 96-bit window that starts with the
    21-bit preamble 0x1f2a60 and whose 75-bit codeword is correctable (BCH, single-bit errors corrected)."""
    name = "SCMFramerBlock"
    _op, _frame_type = "scmframer", types.SCMFrameType


class SCMPlusFramerBlock(_ERTFramerBlock):
    """radio/blocks/protocol/scmplusframer.lua. SCMPlusFramerBlock(): Bit -> SCMPlusFrameType, one 16-byte record per 128-bit window that
    starts with the sync word 0x16a3, whose 112-bit codeword is correctable and whose protocol id is 0x1e."""
    name = "SCMPlusFramerBlock"
    _op, _frame_type = "scmplusframer", types.SCMPlusFrameType


class IDMFramerBlock(_ERTFramerBlock):
    """radio/blocks/protocol/idmframer.lua. IDMFramerBlock(): Bit -> IDMFrameType, one 88-byte record per 736-bit window that starts with the
    preamble 0x5555 and the sync word 0x16a3, whose 704-bit codeword is correctable, whose packet type and length are 0x1c and 0x5cc6 and whose
    serial CRC matches."""
    name = "IDMFramerBlock"
    _op, _frame_type = "idmframer", types.IDMFrameType


class _PacketFramerBlock(_ERTFramerBlock):
    """The two packet framers (luaradio_amd/csrc/stage_framers.h): Bit -> one fixed record per frame, whose type's
    frames() gives the reference's variable-length objects back."""


class AX25FramerBlock(_PacketFramerBlock):
    """radio/blocks/protocol/ax25framer.lua. AX25FramerBlock(): Bit -> AX25FrameType, one 416-byte record per frame between two 0x7e flags whose
    unstuffed length is a whole number of octets (15 .. 398 with the FCS), whose FCS matches and whose address chain, control octet and
    optional PID / payload extract.  As in the reference a frame that shares its opening flag with the closing flag of an emitted frame is
    lost.  The output is the same however the stream is cut into calls."""
    name = "AX25FramerBlock"
    _op, _frame_type = "ax25framer", types.AX25FrameType


class POCSAGFramerBlock(_PacketFramerBlock):
    """radio/blocks/protocol/pocsagframer.lua. POCSAGFramerBlock(): Bit -> POCSAGFrameType, one 256-byte record per frame (address, func and up
    to 62 data words; a longer frame is a chain of records linked by `flags`).  The block is eager: it takes every step of the reference's
    automaton that the bits seen so far allow, so its output does not depend on how the stream is cut into calls, while the reference may
    hold frames back until up to 543 further bits arrive.  reset() drops the pending frame and the buffered bits."""
    name = "POCSAGFramerBlock"
    _op, _frame_type = "pocsagframer", types.POCSAGFrameType


# ---- the Bit -> sample blocks (luaradio_amd/csrc/stage_modulator.h)
MODULATOR_MAX_BITS = 16                     # MOD_MAX_BITS: the symbol table holds at most 2^16 entries


def _symbol_bits(count, what):
    """log2 of `levels` / `points`, with the reference's assertion (pulseamplitudemodulator.lua:37) and the library's table limit"""
    ok = isinstance(count, (int, float, np.integer, np.floating)) and not isinstance(count, bool) and count > 1 and int(count) == count and \
        (int(count) & (int(count) - 1)) == 0
    assert ok, "%s is not greater than 1 and a power of 2" % what
    bits = int(count).bit_length() - 1
    if bits > MODULATOR_MAX_BITS:
        raise ValueError("%s = %d needs a symbol table above the limit of 2^%d entries" % (what, int(count), MODULATOR_MAX_BITS))
    return bits


def _symbol_period(symbol_rate, sample_rate):
    period = int(math.floor(sample_rate / symbol_rate))      # pulseamplitudemodulator.lua:40: from the arguments, not from the block's rate
    if period < 1:
        raise ValueError("symbol period floor(sample_rate / symbol_rate) = %d is below one sample" % period)
    return period


def _symbol_table(custom, size, option):
    """options.amplitudes / options.constellation: a dict or a sequence indexed by symbol value -> list of `size` entries"""
    if isinstance(custom, dict):
        missing = [v for v in range(size) if v not in custom]
        if missing:
            raise ValueError("%s has no entry for symbol value %d" % (option, missing[0]))
        return [custom[v] for v in range(size)]
    entries = list(custom)
    if len(entries) < size:
        raise ValueError("%s has no entry for symbol value %d" % (option, len(entries)))
    return entries[:size]


def pam_amplitudes(levels):
    """PulseAmplitudeModulatorBlock:_build_amplitudes (pulseamplitudemodulator.lua:47-55): Gray-mapped, unit mean energy; computed in double and
    rounded once to Float32 (:62)"""
    scaling = math.sqrt((levels ** 2 - 1) / 3)
    table = np.zeros(levels, np.float32)
    for level in range(levels):
        table[level ^ (level >> 1)] = np.float32((2 * level - levels + 1) / scaling)
    return table


def qam_constellation(points):
    """QuadratureAmplitudeModulatorBlock:_build_constellation (quadratureamplitudemodulator.lua:47-67).  The integer grid point is exact in
    ComplexFloat32; scalar_div (complexfloat32.lua:141-143) divides each component by the double scaling and rounds once to Float32."""
    symbol_bits = int(points).bit_length() - 1
    q_bits = symbol_bits - (symbol_bits + 1) // 2
    i_levels, q_levels = 2 ** (symbol_bits - q_bits), 2 ** q_bits
    scaling = math.sqrt(2 * (points - 1) / 3)
    table = np.zeros(points, np.complex64)
    for point in range(points):
        i_value, q_value = point >> q_bits, point & (q_levels - 1)
        gray = ((i_value ^ (i_value >> 1)) << q_bits) | (q_value ^ (q_value >> 1))
        re, im = np.float32(2 * i_value - i_levels + 1), np.float32(2 * q_value - q_levels + 1)
        table[gray] = complex(np.float32(float(re) / scaling), np.float32(float(im) / scaling))
    return table


class _SymbolMapBlock(Block):
    """what the modulators and the demodulators share: the arguments, their assertions, and the symbol table"""
    _op, _sample, _count_name, _table_option = None, None, None, None

    def _symbol_arguments(self, symbol_rate, sample_rate, count, options):
        assert symbol_rate is not None, "Missing argument #1 (symbol_rate)"
        assert sample_rate is not None, "Missing argument #2 (sample_rate)"
        assert count is not None, "Missing argument #3 (%s)" % self._count_name.lower()
        self.symbol_rate, self.sample_rate, self.options = symbol_rate, sample_rate, dict(options or {})
        self.symbol_bits = _symbol_bits(count, self._count_name)
        self.symbol_period = _symbol_period(symbol_rate, sample_rate)
        msb_first = self.options.get("msb_first")
        self.msb_first = True if msb_first is None else bool(msb_first)

    def _default_table(self):
        raise NotImplementedError

    def table(self):
        """the symbol table as the sample type's vector, indexed by symbol value"""
        custom = self.options.get(self._table_option)
        if custom is None:
            return self._default_table()
        entries = _symbol_table(custom, 1 << self.symbol_bits, self._table_option)
        if self._sample is types.ComplexFloat32:
            entries = [complex(*e) if isinstance(e, (list, tuple)) else complex(e) for e in entries]
            return np.array([complex(np.float32(e.real), np.float32(e.imag)) for e in entries], np.complex64)
        return np.array([np.float32(e) for e in entries], np.float32)


class _ModulatorBlock(_SymbolMapBlock):
    _out = None
    _sample = property(lambda self: self._out)

    def instantiate(self, symbol_rate, sample_rate, count, options=None):
        self._symbol_arguments(symbol_rate, sample_rate, count, options)
        self.add_type_signature([Input("in", types.Bit)], [Output("out", self._out)])

    def op(self):
        values = self.table().view(np.float32)
        return "%s:period=%d:bits=%d:msb=%d:table=%s" % (self._op, self.symbol_period, self.symbol_bits, int(self.msb_first),
                                                        ",".join("%.9g" % float(v) for v in values))

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % self._op)

    def process(self, x):
        return self._execute(x, self._out.dtype)


class PulseAmplitudeModulatorBlock(_ModulatorBlock):
    """radio/blocks/signal/pulseamplitudemodulator.lua. PulseAmplitudeModulatorBlock(symbol_rate, sample_rate, levels[, options]): Bit -> Float32.
    log2(levels) bits make a symbol, its amplitude is held for floor(sample_rate / symbol_rate) samples; bits that do not fill a symbol wait for the
    next call.  options: msb_first (default True), amplitudes (dict or sequence indexed by symbol value).  As in the reference the block does not
    change the rate it reports: a rate-dependent block behind it is given the sample rate by its caller."""
    name = "PulseAmplitudeModulatorBlock"
    _op, _out, _count_name, _table_option = "pam", types.Float32, "Levels", "amplitudes"

    def instantiate(self, symbol_rate, sample_rate, levels, options=None):
        _ModulatorBlock.instantiate(self, symbol_rate, sample_rate, levels, options)
        self.levels = int(levels)

    def _default_table(self):
        return pam_amplitudes(self.levels)


class QuadratureAmplitudeModulatorBlock(_ModulatorBlock):
    """radio/blocks/signal/quadratureamplitudemodulator.lua. QuadratureAmplitudeModulatorBlock(symbol_rate, sample_rate, points[, options]):
    Bit -> ComplexFloat32, as the pulse amplitude modulator with a constellation.  options: msb_first (default True), constellation (dict or
    sequence indexed by symbol value; entries complex numbers or (re, im) pairs)."""
    name = "QuadratureAmplitudeModulatorBlock"
    _op, _out, _count_name, _table_option = "qam", types.ComplexFloat32, "Points", "constellation"

    def instantiate(self, symbol_rate, sample_rate, points, options=None):
        _ModulatorBlock.instantiate(self, symbol_rate, sample_rate, points, options)
        self.points = int(points)

    def _default_table(self):
        return qam_constellation(self.points)


# ---- the sample -> Bit / LLR blocks (luaradio_amd/csrc/stage_demodulator.h)
DEMODULATOR_GENERAL_MAX_BITS = 12           # DEM_GENERAL_MAX_BITS: a table that is no grid is searched from LDS, 2^12 entries at most


def scaled_symbol_table(table, scale):
    """the received constellation scale * table: per component Float32(double(entry) * scale), rounded once"""
    values = (np.ascontiguousarray(table).view(np.float32).astype(np.float64) * float(scale)).astype(np.float32)
    return values.view(table.dtype)


def constellation_grid_bits(table):
    """the smallest qb in 0 .. b with table[v] == (I[v >> qb], Q[v & (2^qb - 1)]) bit for bit for every symbol value v, or None: the demodulator
    then decides each axis on its own (stage_demodulator.h).  Every default qam_constellation is such a grid."""
    table = np.ascontiguousarray(table, np.complex64)
    words = table.view(np.uint32).reshape(-1, 2)
    v = np.arange(len(table))
    for qb in range(len(table).bit_length()):
        if np.array_equal(words[:, 0], words[v >> qb << qb, 0]) and np.array_equal(words[:, 1], words[v & ((1 << qb) - 1), 1]):
            return qb
    return None


class _DemodulatorBlock(_SymbolMapBlock):
    def instantiate(self, symbol_rate, sample_rate, count, options=None):
        self._symbol_arguments(symbol_rate, sample_rate, count, options)
        offset = self.options.get("offset", 0)
        if isinstance(offset, bool) or int(offset) != offset or not 0 <= offset < self.symbol_period:
            raise ValueError("offset = %r is not an integer in 0 .. %d (the symbol period less one)" % (offset, self.symbol_period - 1))
        self.offset = int(offset)
        self.scale = float(self.options.get("scale", 1.0))
        if not math.isfinite(self.scale):
            raise ValueError("scale = %r is not finite" % self.scale)
        self.soft = bool(self.options.get("soft", False))
        noise_variance = self.options.get("noise_variance")
        if noise_variance is not None and not self.soft:
            raise ValueError("noise_variance is the weight of the soft decisions: it needs soft = True")
        self.noise_variance = 1.0 if noise_variance is None else float(noise_variance)
        if not self.noise_variance > 0:
            raise ValueError("noise_variance = %r is not greater than 0" % self.noise_variance)
        with np.errstate(over="ignore"):
            self.weight = np.float32(1.0 / self.noise_variance)
        if not (np.isfinite(self.weight) and self.weight > 0):
            raise ValueError("noise_variance = %r gives no finite Float32 weight above 0" % self.noise_variance)
        self.add_type_signature([Input("in", self._sample)], [Output("out", types.Float32 if self.soft else types.Bit)])

    def received_table(self):
        """scale * table, what the stage compares the samples with"""
        return scaled_symbol_table(self.table(), self.scale)

    def grid(self):
        """the op string's grid field: 1 for the one axis of pam; for qam the low bits of the second axis, -1 for a table that is no grid"""
        if self._sample is types.Float32:
            return 1
        qb = constellation_grid_bits(self.received_table())
        if qb is None and self.symbol_bits > DEMODULATOR_GENERAL_MAX_BITS:
            raise ValueError("%s = %d: a %s that is no grid is limited to 2^%d entries" % (self._count_name, 1 << self.symbol_bits, self._table_option,
                                                                                          DEMODULATOR_GENERAL_MAX_BITS))
        return -1 if qb is None else qb

    def op(self, grid=None):
        """grid = -1 runs a grid-shaped table through the general search (the tests compare the two forms that way)"""
        values = self.received_table().view(np.float32)
        return "%s:period=%d:offset=%d:bits=%d:msb=%d:soft=%d:weight=%.9g:grid=%d:table=%s" % (
            self._op, self.symbol_period, self.offset, self.symbol_bits, int(self.msb_first), int(self.soft), float(self.weight),
            self.grid() if grid is None else grid, ",".join("%.9g" % float(v) for v in values))

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % self._op)

    def process(self, x):
        return self._execute(x, np.float32 if self.soft else np.uint8)


class PulseAmplitudeDemodulatorBlock(_DemodulatorBlock):
    """PulseAmplitudeDemodulatorBlock(symbol_rate, sample_rate, levels[, options]): Float32 -> Bit, the inverse of PulseAmplitudeModulatorBlock (no
    block of the reference).  Symbol s is decided on input sample s P + offset, P = floor(sample_rate / symbol_rate), by the nearest amplitude (ties:
    the lowest symbol value) and leaves as log2(levels) bits.  options: msb_first, amplitudes (as the modulator's); offset (0 .. P - 1, default 0);
    scale (default 1.0: the received amplitudes are scale * amplitudes); soft (default False; True: Float32 max-log LLRs in place of the bits, in the same
    order, positive = bit 0); noise_variance (default 1.0, with soft only: the LLRs are weighted by 1 / noise_variance).  As the modulators, the block
    does not change the rate it reports."""
    name = "PulseAmplitudeDemodulatorBlock"
    _op, _sample, _count_name, _table_option = "pamdemod", types.Float32, "Levels", "amplitudes"

    def instantiate(self, symbol_rate, sample_rate, levels, options=None):
        _DemodulatorBlock.instantiate(self, symbol_rate, sample_rate, levels, options)
        self.levels = int(levels)

    def _default_table(self):
        return pam_amplitudes(self.levels)


class QuadratureAmplitudeDemodulatorBlock(_DemodulatorBlock):
    """QuadratureAmplitudeDemodulatorBlock(symbol_rate, sample_rate, points[, options]): ComplexFloat32 -> Bit (Float32 with soft), as the pulse
    amplitude demodulator with a constellation (option constellation, as the modulator's).  A constellation that is a grid of two axes - every default
    one - is decided per axis; any other one of up to 2^12 points by a search over all points."""
    name = "QuadratureAmplitudeDemodulatorBlock"
    _op, _sample, _count_name, _table_option = "qamdemod", types.ComplexFloat32, "Points", "constellation"

    def instantiate(self, symbol_rate, sample_rate, points, options=None):
        _DemodulatorBlock.instantiate(self, symbol_rate, sample_rate, points, options)
        self.points = int(points)

    def _default_table(self):
        return qam_constellation(self.points)


# ---- forward error correction (luaradio_amd/csrc/stage_viterbi.h): a rate-1/n convolutional code and its windowed Viterbi decoder
def _is_integer(v):
    """an int or a numpy integer, and no bool"""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_convolutional_code(who, constraint_length, polynomials):
    """the checks both blocks share; the library makes them again on the op string.  Returns (K, [g_0, ...])"""
    K = constraint_length
    if not (_is_integer(K) and 3 <= K <= 9):
        raise ValueError("%s: constraint length must be 3 .. 9 (got %r)" % (who, K))
    try:
        polys = list(polynomials)
    except TypeError:
        raise ValueError("%s: polynomials must be a list of integers (got %r)" % (who, polynomials))
    for g in polys:
        if not _is_integer(g):
            raise ValueError("%s: polynomials must be integers (got %r)" % (who, g))
    polys = [int(g) for g in polys]
    if not 2 <= len(polys) <= 4:
        raise ValueError("%s: the number of polynomials must be 2 .. 4 (got %d)" % (who, len(polys)))
    for g in polys:
        if g < 0 or g >> K:
            raise ValueError("%s: polynomial %s (octal) has bits at or above the constraint length %d" % (who, ("%o" % g) if g >= 0 else g, K))
    text = ",".join("%o" % g for g in polys)
    if not any((g >> (K - 1)) & 1 for g in polys):
        raise ValueError("%s: no polynomial of %s has bit %d set: the current input bit reaches no output" % (who, text, K - 1))
    if not any(g & 1 for g in polys):
        raise ValueError("%s: no polynomial of %s has bit 0 set: the constraint length is below %d" % (who, text, K))
    return int(K), polys


class ConvolutionalEncoderBlock(Block):
    """ConvolutionalEncoderBlock(constraint_length, polynomials): Bit -> Bit, n = len(polynomials) output bits per input bit.  Not a block of the
    reference.  K = constraint_length is 3 .. 9, n is 2 .. 4, and the polynomials are integers in the usual octal notation, bit K - 1 multiplying
    the current input bit: ConvolutionalEncoderBlock(7, [0o171, 0o133]) is the code of DVB-S, 802.11a and CCSDS.  The register starts at zero at
    bit 0 of the stream; r = (u << (K - 1)) | (r >> 1), out[n t + j] = parity(r & g_j)."""
    name = "ConvolutionalEncoderBlock"

    def instantiate(self, constraint_length, polynomials):
        assert constraint_length is not None, "Missing argument #1 (constraint_length)"
        assert polynomials is not None, "Missing argument #2 (polynomials)"
        self.constraint_length, self.polynomials = check_convolutional_code("convenc", constraint_length, polynomials)
        self.add_type_signature([Input("in", types.Bit)], [Output("out", types.Bit)])

    def get_rate(self):
        return Block.get_rate(self) * len(self.polynomials)

    def op(self):
        """the stage as lrhip_unary_create takes it; the polynomials are octal text"""
        return "convenc:k=%d:polys=%s" % (self.constraint_length, ",".join("%o" % g for g in self.polynomials))

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip convenc object")

    def process(self, x):
        return self._execute(x, np.uint8)


class ViterbiDecoderBlock(Block):
    """ViterbiDecoderBlock(constraint_length, polynomials[, options]): Float32 LLRs -> Bit, or Bit -> Bit; the decoder of ConvolutionalEncoderBlock.
    Not a block of the reference.
    options = {"soft": True - the input is Float32 LLRs in the demodulators' convention, POSITIVE MEANS 0; False - Bit, a bit b counting as the
               saturated value 127 (1 - 2 b);
               "scale": 8.0 - an LLR is quantised once to clamp(rint(llr * scale), -127, 127), NaN to 0 (an erasure);
               "block": D = 512 decoded bits per window, 64 .. 2048;
               "depth": L = 8 (K - 1) steps, K - 1 .. 256: the acquisition length in front of a window and the traceback tail behind it}
    with (D + 2 L) 2^(K - 1) / 8 <= 65536 bytes of decisions per window.
    A sliding-window decoder on absolute step indices: window w decodes the bits [w D, (w + 1) D) from the steps max(0, w D - L) ..
    (w + 1) D + L - 1 of the stream, so the output is a function of the stream alone - any chunking, reset, seek or time partition gives the same
    bits - and a call returns the windows its inputs complete, possibly none.  THERE IS NO FLUSH: the last fewer than D + L bits of a stream are
    never emitted; pad the stream with n (D + L) zero LLRs (erasures) to get them.  luaradio_amd/csrc/kernels_viterbi.h has the arithmetic."""
    name = "ViterbiDecoderBlock"

    def instantiate(self, constraint_length, polynomials, options=None):
        assert constraint_length is not None, "Missing argument #1 (constraint_length)"
        assert polynomials is not None, "Missing argument #2 (polynomials)"
        options = options or {}
        K, self.polynomials = check_convolutional_code("viterbi", constraint_length, polynomials)
        self.constraint_length = K
        self.soft = bool(options.get("soft", True))
        scale = options.get("scale", 8.0)
        try:
            self.scale = np.float32(scale)
        except (TypeError, ValueError):
            raise ValueError("viterbi: scale must be a finite Float32 above 0 (got %r)" % (scale,))
        if not (np.isfinite(self.scale) and self.scale > 0):
            raise ValueError("viterbi: scale must be a finite Float32 above 0 (got %r)" % (scale,))
        self.block = options.get("block", 512)
        if not (_is_integer(self.block) and 64 <= self.block <= 2048):
            raise ValueError("viterbi: block must be 64 .. 2048 decoded bits (got %r)" % (self.block,))
        self.depth = options.get("depth", 8 * (K - 1))
        if not (_is_integer(self.depth) and K - 1 <= self.depth <= 256):
            raise ValueError("viterbi: depth must be %d .. 256 steps (got %r)" % (K - 1, self.depth))
        nbytes = (self.block + 2 * self.depth) * (1 << (K - 1)) // 8
        if nbytes > 65536:
            raise ValueError("viterbi: the decision words of one window, (block + 2 depth) * 2^(k - 1) / 8 = %d bytes, exceed 65536: "
                             "use a smaller block or depth" % nbytes)
        self.add_type_signature([Input("in", types.Float32 if self.soft else types.Bit)], [Output("out", types.Bit)])

    def get_rate(self):
        return Block.get_rate(self) / len(self.polynomials)

    def memory(self):
        """inputs after which a decoder started by seek() emits what the uninterrupted stream would"""
        return len(self.polynomials) * (self.block + 2 * self.depth) - 1

    def op(self):
        """the stage as lrhip_unary_create takes it; the polynomials are octal text, %.9g gives the Float32 scale back exactly"""
        return "viterbi:k=%d:polys=%s:input=%s:scale=%.9g:block=%d:depth=%d" % (self.constraint_length, ",".join("%o" % g for g in self.polynomials),
                                                                            "llr" if self.soft else "bit", float(self.scale), self.block, self.depth)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip viterbi object")

    def process(self, x):
        return self._execute(x, np.uint8)


# ---- Reed-Solomon codes over GF(2^8) and the Bit <-> Byte stages around them (luaradio_amd/csrc/stage_reedsolomon.h)
def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def is_primitive_polynomial(gfpoly):
    """degree 8 over GF(2), and alpha = 2 has order 255 modulo it (16 polynomials, 0x11d the first)"""
    if not (_is_integer(gfpoly) and 0x100 <= gfpoly <= 0x1ff):
        return False
    x, seen = 1, set()
    for _ in range(255):
        if x == 0 or x in seen:
            return False
        seen.add(x)
        x <<= 1
        if x & 0x100:
            x ^= int(gfpoly)
    return x == 1


def check_reed_solomon_code(who, n, k, options):
    """the checks both blocks share; the library makes them again on the op string.  Returns (n, k, gfpoly, fcr, prim, interleave)"""
    unknown = sorted(set(options) - {"gfpoly", "fcr", "prim", "interleave", "status"})
    if unknown or ("status" in options and who != "rsdec"):
        raise ValueError("%s: unknown option %r" % (who, unknown[0] if unknown else "status"))
    if not (_is_integer(n) and 3 <= n <= 255):
        raise ValueError("%s: n must be 3 .. 255 (got %r)" % (who, n))
    if not (_is_integer(k) and 1 <= k < n and (n - k) % 2 == 0 and 2 <= n - k <= 64):
        raise ValueError("%s: k must be 1 .. n - 2 with n - k even and 2 .. 64 (got n = %r, k = %r)" % (who, n, k))
    gfpoly, fcr, prim, interleave = (options.get("gfpoly", 0x11d), options.get("fcr", 0), options.get("prim", 1), options.get("interleave", 1))
    if not is_primitive_polynomial(gfpoly):
        raise ValueError("%s: gfpoly %s is not a primitive polynomial of degree 8" % (who, hex(gfpoly) if _is_integer(gfpoly) else repr(gfpoly)))
    if not (_is_integer(fcr) and 0 <= fcr <= 254):
        raise ValueError("%s: fcr must be 0 .. 254 (got %r)" % (who, fcr))
    if not (_is_integer(prim) and 1 <= prim <= 254 and _gcd(int(prim), 255) == 1):
        raise ValueError("%s: prim must be 1 .. 254 and coprime to 255 (got %r)" % (who, prim))
    if not (_is_integer(interleave) and 1 <= interleave <= 8):
        raise ValueError("%s: interleave must be 1 .. 8 (got %r)" % (who, interleave))
    return int(n), int(k), int(gfpoly), int(fcr), int(prim), int(interleave)


class _FramedBlock(Block):
    """a stage of whole frames: frame_in input bytes give frame_out output bytes.  Everything is a function of the absolute input index - any
    chunking, reset, seek or time partition gives the same bytes -, a call returns the frames its input completes, possibly none, and there is no
    flush.  seek(n0) lands on frame n0 // frame_in and counts the bytes of that frame in front of n0 as zeros."""
    frame_in = frame_out = 1

    def get_rate(self):
        return Block.get_rate(self) * self.frame_out / self.frame_in

    def memory(self):
        """inputs after which a stage started by seek() emits what the uninterrupted stream would"""
        return self.frame_in - 1

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % self.op().split(":")[0])

    def process(self, x):
        return self._execute(x, np.uint8)


class ReedSolomonEncoderBlock(_FramedBlock):
    """ReedSolomonEncoderBlock(n, k[, options]): Byte -> Byte, a systematic Reed-Solomon code over GF(2^8) in the conventional (polynomial) basis.
    Not a block of the reference.
    options = {"gfpoly": 0x11d - the field polynomial, one of the 16 primitive polynomials of degree 8; alpha = 2 is a root of it;
               "fcr": 0 - the first consecutive root, 0 .. 254;
               "prim": 1 - the root spacing, 1 .. 254 and coprime to 255: g(x) = prod_{i < n - k} (x - alpha^((fcr + i) prim));
               "interleave": 1 - I = 1 .. 8 codewords per frame, symbol-interleaved as in CCSDS}
    n <= 255, k >= 1, n - k even and 2 .. 64 (t = (n - k) / 2 = 1 .. 32); n < 255 is the shortened code, its 255 - n virtual bytes zeros at the
    highest degrees.  Byte j of a codeword is the coefficient of x^(n - 1 - j): the k message bytes first, unchanged, then n - k parity bytes.  A
    frame is I k bytes in and I n bytes out; byte j of a frame belongs to codeword j mod I at index j div I; the output frame is the I k message
    bytes as they came, then the I (n - k) parity bytes interleaved the same way.
    DVB-S: ReedSolomonEncoderBlock(204, 188) (gfpoly 0x11d, fcr 0, prim 1).  CCSDS: ReedSolomonEncoderBlock(255, 223, {"gfpoly": 0x187,
    "fcr": 112, "prim": 11, "interleave": 1 .. 5}) - in the conventional basis: the dual-basis symbol representation of CCSDS is not applied."""
    name = "ReedSolomonEncoderBlock"
    _who = "rsenc"

    def instantiate(self, n, k, options=None):
        assert n is not None, "Missing argument #1 (n)"
        assert k is not None, "Missing argument #2 (k)"
        options = options or {}
        self.n, self.k, self.gfpoly, self.fcr, self.prim, self.interleave = check_reed_solomon_code(self._who, n, k, options)
        self.t = (self.n - self.k) // 2
        self._frames(options)
        self.add_type_signature([Input("in", types.Byte)], [Output("out", types.Byte)])

    def _frames(self, options):
        self.frame_in, self.frame_out = self.interleave * self.k, self.interleave * self.n

    def op(self):
        """the stage as lrhip_unary_create takes it; gfpoly is decimal text"""
        return "%s:n=%d:k=%d:gfpoly=%d:fcr=%d:prim=%d:interleave=%d" % (self._who, self.n, self.k, self.gfpoly, self.fcr, self.prim, self.interleave)


class ReedSolomonDecoderBlock(ReedSolomonEncoderBlock):
    """ReedSolomonDecoderBlock(n, k[, options]): Byte -> Byte, the decoder of ReedSolomonEncoderBlock, with its options and
              "status": False - True: the I k message bytes of a frame are followed by I status bytes, one per codeword.
    A frame is I n bytes in and I k corrected message bytes out, in the interleaved order they arrived in.  Bounded-distance decoding: a codeword
    within Hamming distance t of the received word is found and returned, and its status is the number of symbols corrected, 0 .. t (corrections in
    parity bytes count).  Otherwise the word is uncorrectable - the locator's register is longer than t, the locator does not have exactly that
    many roots among the n real positions (a root in the virtual pad of a shortened code is no position), or an error magnitude comes out zero -:
    its status is 255 and its message bytes leave as received.  There is no erasure input (symbols the demodulator flags as unreliable): out of scope."""
    name = "ReedSolomonDecoderBlock"
    _who = "rsdec"

    def _frames(self, options):
        self.status = bool(options.get("status", False))
        self.frame_in, self.frame_out = self.interleave * self.n, self.interleave * (self.k + (1 if self.status else 0))

    def op(self):
        return ReedSolomonEncoderBlock.op(self) + ":status=%d" % self.status


class PackBitsBlock(_FramedBlock):
    """PackBitsBlock([options]): Bit -> Byte, eight bits per byte on absolute bit indices; options = {"order": "msb" - the first bit is the most
    significant one; "lsb"}.  Bit 0 of each input byte is read; up to 7 bits are carried between calls.  Not a block of the reference."""
    name = "PackBitsBlock"
    _who, frame_in, frame_out, _types = "packbits", 8, 1, (types.Bit, types.Byte)

    def instantiate(self, options=None):
        options = options or {}
        unknown = sorted(set(options) - {"order"})
        if unknown:
            raise ValueError("%s: unknown option %r" % (self._who, unknown[0]))
        self.order = options.get("order", "msb")
        if self.order not in ("msb", "lsb"):
            raise ValueError("%s: unsupported order %r (msb or lsb)" % (self._who, self.order))
        self.add_type_signature([Input("in", self._types[0])], [Output("out", self._types[1])])

    def op(self):
        return "%s:order=%s" % (self._who, self.order)


class UnpackBitsBlock(PackBitsBlock):
    """UnpackBitsBlock([options]): Byte -> Bit, eight bits per byte, stateless; options as PackBitsBlock.  Not a block of the reference."""
    name = "UnpackBitsBlock"
    _who, frame_in, frame_out, _types = "unpackbits", 1, 8, (types.Byte, types.Bit)


# ---- puncturing, the Forney interleaver and the additive scrambler (luaradio_amd/csrc/stage_fecglue.h): what joins the convolutional and the
# Reed-Solomon stages into a standard concatenated link.  dvbs_fec_encoder / dvbs_fec_decoder in composites.py are the DVB-S chain.
def check_puncture_pattern(who, pattern):
    """the checks both blocks share; the library makes them again on the op string"""
    if not isinstance(pattern, str) or set(pattern) - set("01"):
        raise ValueError("%s: pattern must be a string of 0 / 1 characters, got %r" % (who, pattern))
    if not 2 <= len(pattern) <= 64:
        raise ValueError("%s: pattern must be 2 .. 64 characters (got %d)" % (who, len(pattern)))
    if "1" not in pattern:
        raise ValueError("%s: pattern must not be all 0 (got %r)" % (who, pattern))
    return pattern


class PunctureBlock(_FramedBlock):
    """PunctureBlock(pattern): Bit -> Bit.  pattern is 2 .. 64 characters 0 / 1 with at least one 1; a frame is len(pattern) elements in and
    pattern.count("1") out, element j of a frame kept where pattern[j] == "1".  Bytes are moved, never interpreted.  Behind
    ConvolutionalEncoderBlock(7, [0o171, 0o133]) the patterns of composites.DVBS_PUNCTURE give the DVB-S rates.  Not a block of the reference."""
    name = "PunctureBlock"
    _who = "puncture"

    def instantiate(self, pattern):
        assert pattern is not None, "Missing argument #1 (pattern)"
        self.pattern = check_puncture_pattern(self._who, pattern)
        self.frame_in, self.frame_out = len(pattern), pattern.count("1")
        self.add_type_signature([Input("in", types.Bit)], [Output("out", types.Bit)])

    def op(self):
        return "puncture:pattern=%s" % self.pattern


class DepunctureBlock(_FramedBlock):
    """DepunctureBlock(pattern[, options]): Float32 -> Float32, or Bit -> Float32 with options = {"soft": False}; the inverse framing of
    PunctureBlock: pattern.count("1") elements in, len(pattern) Float32 out, +0.0 where pattern[j] == "0" - the LLR ViterbiDecoderBlock counts as an
    erasure.  soft (the default): the LLRs are moved as their 32 bits, a NaN stays that NaN.  Bit: bit 0 of the input byte is read, 0 gives +1.0 and
    1 gives -1.0, the demodulators' sign convention, so that ViterbiDecoderBlock(..., {"scale": 127}) behind it sees exactly its hard input.
    Not a block of the reference."""
    name = "DepunctureBlock"
    _who = "depuncture"

    def instantiate(self, pattern, options=None):
        assert pattern is not None, "Missing argument #1 (pattern)"
        options = options or {}
        unknown = sorted(set(options) - {"soft"})
        if unknown:
            raise ValueError("depuncture: unknown option %r" % (unknown[0],))
        self.pattern = check_puncture_pattern(self._who, pattern)
        self.soft = bool(options.get("soft", True))
        self.frame_in, self.frame_out = pattern.count("1"), len(pattern)
        self.add_type_signature([Input("in", types.Float32 if self.soft else types.Bit)], [Output("out", types.Float32)])

    def op(self):
        return "depuncture:pattern=%s:input=%s" % (self.pattern, "llr" if self.soft else "bit")

    def process(self, x):
        return self._execute(x, np.float32)


class ConvolutionalInterleaverBlock(Block):
    """ConvolutionalInterleaverBlock(branches, step): Byte -> Byte, the convolutional (Forney) interleaver with I = branches = 2 .. 256 and
    M = step = 1 .. 256, depth D = (I - 1) M I <= 65536: with j = i mod I on the absolute byte index i, out[i] = in[i - j M I], in[negative] = 0 (the
    zero-filled FIFOs of the standards).  ConvolutionalDeinterleaverBlock undoes it up to a delay of D bytes.  DVB-S: (12, 17), D = 2244 bytes = 11
    packets of 204; the sync bytes, at multiples of 204, ride branch 0 and are not delayed.  The last D input bytes are carried between calls;
    seek(n0) continues at output n0 with zeros for everything in front.  Not a block of the reference."""
    name = "ConvolutionalInterleaverBlock"
    _who = "convinterleave"

    def instantiate(self, branches, step):
        assert branches is not None, "Missing argument #1 (branches)"
        assert step is not None, "Missing argument #2 (step)"
        if not (_is_integer(branches) and 2 <= branches <= 256):
            raise ValueError("%s: branches must be 2 .. 256 (got %r)" % (self._who, branches))
        if not (_is_integer(step) and 1 <= step <= 256):
            raise ValueError("%s: step must be 1 .. 256 (got %r)" % (self._who, step))
        self.branches, self.step = int(branches), int(step)
        self.depth = (self.branches - 1) * self.step * self.branches
        if self.depth > 65536:
            raise ValueError("%s: the depth (branches - 1) * step * branches = %d must be at most 65536" % (self._who, self.depth))
        self.add_type_signature([Input("in", types.Byte)], [Output("out", types.Byte)])

    def memory(self):
        """inputs after which a stage started by seek() emits what the uninterrupted stream would"""
        return self.depth

    def op(self):
        return "%s:branches=%d:step=%d" % (self._who, self.branches, self.step)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % self._who)

    def process(self, x):
        return self._execute(x, np.uint8)


class ConvolutionalDeinterleaverBlock(ConvolutionalInterleaverBlock):
    """ConvolutionalDeinterleaverBlock(branches, step): Byte -> Byte, out[i] = in[i - (I - 1 - j) M I] with j = i mod I; behind
    ConvolutionalInterleaverBlock(branches, step) the stream comes back delayed by D = (I - 1) M I bytes, the first D outputs zeros.  Both streams
    count from the same byte 0: there is no search for the branch phase.  Not a block of the reference."""
    name = "ConvolutionalDeinterleaverBlock"
    _who = "convdeinterleave"


def lfsr_sequence(taps, seed_bits, nbits):
    """nbits bits (a multiple of 8) of the linear recurrence s[m] = xor of s[m - i] for i in taps, from seed_bits[i - 1] = s[-i], packed MSB first
    into a uint8 array: the stuff of AdditiveScramblerBlock tables"""
    taps = [int(t) for t in taps]
    order = max(taps)
    if min(taps) < 1 or len(seed_bits) != order:
        raise ValueError("lfsr_sequence: taps are positive and the seed has max(taps) = %d bits (got %d)" % (order, len(seed_bits)))
    if nbits < 8 or nbits % 8:
        raise ValueError("lfsr_sequence: nbits must be a positive multiple of 8 (got %r)" % (nbits,))
    s = np.zeros(order + nbits, np.uint8)
    s[:order] = [int(b) & 1 for b in reversed(list(seed_bits))]
    for m in range(order, order + nbits):
        v = 0
        for t in taps:
            v ^= s[m - t]
        s[m] = v
    return np.packbits(s[order:])


def dvb_energy_dispersal_table(frame=188):
    """the energy dispersal of EN 300 421 as a table for AdditiveScramblerBlock, one period of 8 transport packets: byte 0 is 0xFF (the sync
    inversion 0x47 -> 0xB8); the PRBS 1 + x^14 + x^15, seed 100101010000000, runs from byte 1; at the seven other sync bytes, 188 q, the entry is 0
    but the PRBS advances.  frame=189: every frame has a 189th entry that is 0 and does not advance the PRBS, for a stream of
    ReedSolomonDecoderBlock(204, 188, {"status": True})"""
    if frame not in (188, 189):
        raise ValueError("dvb_energy_dispersal_table: frame must be 188 or 189 (got %r)" % (frame,))
    prbs = lfsr_sequence((14, 15), [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0], 8 * 1503)
    packets = np.concatenate([[0xFF], prbs]).astype(np.uint8).reshape(8, 188)
    packets[1:, 0] = 0
    table = np.zeros((8, frame), np.uint8)
    table[:, :188] = packets
    return table.ravel()


def ccsds_randomizer_table(nbytes):
    """nbytes of the CCSDS pseudo-randomizer h(x) = x^8 + x^7 + x^5 + x^3 + 1 from the all-ones state (ff 48 0e c0 9a ...; its period is 255 bits).
    A table as long as the transfer frame restarts it at every frame"""
    if not (_is_integer(nbytes) and 1 <= nbytes <= 8192):
        raise ValueError("ccsds_randomizer_table: nbytes must be 1 .. 8192 (got %r)" % (nbytes,))
    taps = (1, 3, 5, 8)
    # the seed whose first eight outputs are ones: the recurrence run backwards from them, s[m - 8] = s[m] ^ s[m - 1] ^ s[m - 3] ^ s[m - 5]
    s = [1] * 8                                                   # s[0 .. 7]; s[-1], s[-2], ... are put in front
    for _ in range(8):
        s.insert(0, s[7] ^ s[6] ^ s[4] ^ s[2])
    return lfsr_sequence(taps, s[7::-1], 8 * int(nbytes))


class AdditiveScramblerBlock(Block):
    """AdditiveScramblerBlock(table[, options]): Byte -> Byte, out[i] = in[i] ^ table[(i + offset) mod P] on the absolute byte index i; the same
    block descrambles.  table is 1 .. 8192 bytes (anything np.asarray turns into integers 0 .. 255), options = {"offset": 0 - 0 .. P - 1}.  The
    device knows no polynomial: lfsr_sequence, dvb_energy_dispersal_table and ccsds_randomizer_table build tables.  Not a block of the reference."""
    name = "AdditiveScramblerBlock"

    def instantiate(self, table, options=None):
        assert table is not None, "Missing argument #1 (table)"
        options = options or {}
        unknown = sorted(set(options) - {"offset"})
        if unknown:
            raise ValueError("scrambler: unknown option %r" % (unknown[0],))
        try:
            values = np.asarray(table)
            ok = values.ndim == 1 and values.dtype.kind in "ui" and values.size > 0 and int(values.min()) >= 0 and int(values.max()) <= 255
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("scrambler: the table must be a vector of integers 0 .. 255")
        if not 1 <= values.size <= 8192:
            raise ValueError("scrambler: the table has %d bytes, it must be 1 .. 8192" % values.size)
        self.table = values.astype(np.uint8)
        self.offset = options.get("offset", 0)
        if not (_is_integer(self.offset) and 0 <= self.offset < len(self.table)):
            raise ValueError("scrambler: offset must be 0 .. %d, the table's length less one (got %r)" % (len(self.table) - 1, self.offset))
        self.offset = int(self.offset)
        self.add_type_signature([Input("in", types.Byte)], [Output("out", types.Byte)])

    def memory(self):
        return 0

    def op(self):
        """the stage as lrhip_unary_create takes it; the table is hexadecimal text, two digits per byte"""
        return "scrambler:table=%s:offset=%d" % (self.table.tobytes().hex(), self.offset)

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip scrambler object")

    def process(self, x):
        return self._execute(x, np.uint8)


# ---- many-ported blocks (luaradio_amd/csrc/stage_interleave.h).  The side of the call with several ports travels as a port table
# (_lib.port_table), the stages run through lrhip_stage_execute_device alone.
MAX_CHANNELS = _lib.MAX_PORTS


def interleave_op(name, num_channels, size):
    return "%s:channels=%d:size=%d" % (name, num_channels, size)


def deinterleave_plan(index, num_channels, n):
    """DeinterleaveBlock's carried index as a rotation of the port table (deinterleave.lua:49-63): for a call of n samples, table entry j
    (the port that receives samples j, j + N, ...) is channel (j + index) mod N.  Returns (channel of every table entry, samples of every
    CHANNEL - the reference's ceil((n - offset) / N) with offset = (channel - index) mod N -, the index after the call)."""
    N = num_channels
    order = [(j + index) % N for j in range(N)]
    counts = [max(0, -(-(n - ((c - index) % N)) // N)) for c in range(N)]
    return order, counts, (index + n) % N


class _Scratch:
    """device vectors of one host-side process() call (lrhip_malloc), freed when the call ends"""

    def __init__(self):
        self.L, self.ptrs = _lib.load(), []

    def alloc(self, nbytes):
        p = _lib.check_ptr(self.L.lrhip_malloc(max(int(nbytes), 16)), "lrhip_malloc")
        self.ptrs.append(p)
        return p

    def upload(self, x):
        import ctypes as C
        p = self.alloc(x.nbytes)
        if x.nbytes:
            _lib.check(self.L.lrhip_memcpy_h2d(p, x.ctypes.data_as(C.c_void_p), x.nbytes), "h2d")
        return p

    def download(self, p, count, dtype):
        import ctypes as C
        y = np.empty(count, dtype)
        if y.nbytes:
            _lib.check(self.L.lrhip_memcpy_d2h(y.ctypes.data_as(C.c_void_p), p, y.nbytes), "d2h")
        return y

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.L.lrhip_free(p)
        self.ptrs = []


class _PortBlock(Block):
    """a block whose stage has several input ports (_many_in) or several output ports"""
    _many_in = True

    def _create(self, op):
        self._op = op
        self._set_stage(_lib.load().lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % op.split(":")[0])

    def process_device_ports(self, ins, n_in, outs, out_capacity):
        """one device call: `ins` and `outs` are lists of device addresses, one per port; the list of the many-ported side becomes the port
        table.  n_in counts samples per input port, out_capacity is the capacity of each output port.  Returns the stage's count."""
        import ctypes as C
        table = _lib.port_table(ins if self._many_in else outs)
        at = C.addressof(table)
        got = _lib.load().lrhip_stage_execute_device(self.stage_handle(), at if self._many_in else ins[0], n_in, outs[0] if self._many_in else at, out_capacity)
        return _lib.check(got, "%s:process_device_ports" % self.name)

    def _same_length(self, xs, dtype):
        xs = [np.ascontiguousarray(x) for x in xs]
        if len(xs) != self.num_channels or any(x.dtype != dtype or len(x) != len(xs[0]) for x in xs):
            raise TypeError("Block %s expects %d %s vectors of equal length" % (self.name, self.num_channels, np.dtype(dtype).name))
        return xs


class InterleaveBlock(_PortBlock):
    """radio/blocks/signal/interleave.lua. InterleaveBlock([num_channels=2]): in1 .. inN (Float32 or ComplexFloat32) -> out,
    out[N i + k] = in_k[i].  The samples are moved as bytes (NaN payloads survive)."""
    name = "InterleaveBlock"

    def instantiate(self, num_channels=2):
        self.num_channels = 2 if num_channels is None else num_channels
        assert self.num_channels > 1, "Number of channels must be greater than 1"
        assert isinstance(self.num_channels, int) and self.num_channels <= MAX_CHANNELS, "Number of channels must be an integer of at most %d" % MAX_CHANNELS
        for t in (types.Float32, types.ComplexFloat32):
            self.add_type_signature([Input("in%d" % (i + 1), t) for i in range(self.num_channels)], [Output("out", t)])

    def op(self):
        return interleave_op("interleave", self.num_channels, self.get_input_type().size)

    def initialize(self):
        self._create(self.op())

    def process(self, *xs):
        dt = self.get_input_type().dtype
        xs = self._same_length(xs, dt)
        n = len(xs[0])
        with _Scratch() as s:
            out = s.alloc(n * self.num_channels * dt.itemsize)
            got = self.process_device_ports([s.upload(x) for x in xs], n, [out], n * self.num_channels)
            return s.download(out, got, dt)


class DeinterleaveBlock(_PortBlock):
    """radio/blocks/signal/deinterleave.lua. DeinterleaveBlock([num_channels=2]): in (Float32 or ComplexFloat32) -> out1 .. outN,
    out_j[i] = in[N i + j] over the whole stream: the position in the frame is carried across calls (`index`, as in the reference) and a
    call may end anywhere in a frame.  process(x) returns a tuple of N vectors, whose lengths differ by at most one."""
    name = "DeinterleaveBlock"
    _many_in = False

    def instantiate(self, num_channels=2):
        self.num_channels = 2 if num_channels is None else num_channels
        assert self.num_channels > 1, "Number of channels must be greater than 1"
        assert isinstance(self.num_channels, int) and self.num_channels <= MAX_CHANNELS, "Number of channels must be an integer of at most %d" % MAX_CHANNELS
        for t in (types.Float32, types.ComplexFloat32):
            self.add_type_signature([Input("in", t)], [Output("out%d" % (i + 1), t) for i in range(self.num_channels)])
        self.index = 0

    def op(self):
        return interleave_op("deinterleave", self.num_channels, self.get_input_type().size)

    def initialize(self):
        self.index = 0
        self._create(self.op())

    def reset(self):
        self.index = 0
        super().reset()

    def max_output(self, n_in):
        return -(-n_in // self.num_channels)

    def process_device_channels(self, in_ptr, n_in, out_ptrs, out_capacity):
        """one device call on the stream: out_ptrs[c] is the vector of CHANNEL c; returns the samples each channel received"""
        order, counts, index = deinterleave_plan(self.index, self.num_channels, n_in)
        if n_in:
            self.process_device_ports([in_ptr], n_in, [out_ptrs[c] for c in order], out_capacity)
        self.index = index
        return counts

    def process(self, x):
        dt = self.get_input_type().dtype
        x = np.ascontiguousarray(x)
        if x.dtype != dt:
            raise TypeError("Block %s expects %s input, got %s" % (self.name, self.get_input_type(), x.dtype))
        cap = self.max_output(len(x))
        with _Scratch() as s:
            outs = [s.alloc(cap * dt.itemsize) for _ in range(self.num_channels)]
            counts = self.process_device_channels(s.upload(x), len(x), outs, cap)
            return tuple(s.download(p, c, dt) for p, c in zip(outs, counts))
