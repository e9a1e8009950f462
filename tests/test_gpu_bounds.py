"""Every device stage and fused chain inside guard words (tests/helpers/guarded.py): no store before `out` or at / after out + count, every sample
of [0, count) written and finite, the input untouched, the same bytes whatever lies next to the input, and the block's existing bar against its oracle.

Each case runs the stream as two consecutive device calls with the lengths n in {1, 3, 2T + 1, 3T - 1, 3T} (T = the outputs of one workgroup or tile of
that form, TILES below; kernels that store 16 bytes per lane also 2T + 2, 2T + 3, so that n mod 4 takes 1, 2, 3) at input and output offsets of 0 and one
sample from a 16-byte boundary (the FIR forms: 0 .. 3 floats; the discriminator: 0, 1, 2 floats out; the record formats: 0 and 1 byte).

The oracle and the bar of check (f) are those of the block's parity test: the C oracle (oracle/oracle.py) where it has the stage, the float64
definition with the golden vectors' epsilon for the element-wise blocks whose parity test is the golden vector alone, the Python models of
tests/helpers for the counted stages, and the unfused device blocks for the fused chains.

FirForm (luaradio_amd/csrc/fir_form.h), each pinned to its shape by a row "bounds: ..." of tools/host_fir_form_check.hip:
  DecFft          test_fir_form[decfft]              OverlapSave     test_fir_fft_form (below)
  WinReal         opt-in knob, not covered           WinCplx         opt-in knob, not covered
  WinShort        test_fir_form[winshort]            WinShortC       test_fir_form[winshortc]
  ShortReal       test_fir_form[shortreal]           WinPair         test_fir_form[winpair]
  DecimLds1       test_fir_form[decimlds1]           DecimLds2       test_fir_form[decimlds2]
  Direct          test_fir_form[direct]              MfmaCc          test_fir_form[mfmacc]
  MfmaPersistent  test_fir_form[persistent-*]        MfmaGeneric     test_fir_form[generic-*]
FirFftForm:
  Pass1024        test_fir_fft_form[*-128, *-512]    Wg4k            test_fir_fft_form[cf32-*-513, cf32-*-1281]
  Long64          test_fir_fft_form[*-1282 .. 4098]  Wave64          test_fir_fft_form[f32-real-513, -1281]; test_fir_fft_large[wave64]
  Pols            test_fir_fft_large[pols]
"""
import ctypes as C
import functools

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from oracle import oracle as O
from tests import golden_util as G
from tests.helpers import guarded as GD

pytestmark = pytest.mark.gpu
RATE = 2.0

# outputs of one workgroup / tile per kernel form, and the line each restates
TILES = {
    "unary4": (1024, "stage_elem3.h:27 items = n / unary_vec_samples(op) = n / 4, one per thread, 256 threads"),
    "unary2": (512, "stage_elem3.h:27 unary_vec_samples(op) = 2 (conjugate, real -> complex, complex add)"),
    "vec4r": (1024, "stage_elem2.h:132 / :191 grid_for(nf4 / 4, 256): 256 float4 of Float32"),
    "vec4c": (512, "stage_elem2.h:132 / :191 the same 256 float4 = 512 ComplexFloat32"),
    "f2c": (512, "stage_elem2.h:123 grid_for(n / 2 + 1, 256): two samples per thread"),
    "upsr": (4096, "stage_elem2.h:232 grid_for(items + 1, 256 * UPS_U), UPS_U = 4 stores of 4 Float32"),
    "upsc": (2048, "stage_elem2.h:230 the same with 2 ComplexFloat32 per store"),
    "one": (256, "one sample per thread, 256 threads (downsample_kernel, delay_kernel, the scalar forms)"),
    "delay4": (1024, "stage_elem3.h:74 grid_for(n4 + D4, 256): 256 float4 = 1024 floats"),
    "rot2": (1024, "stage_elem.h:28 grid_for((n / 2 + 1) / 2 + 1, 256): two float4 = four samples per thread"),
    "disc4": (1024, "stage_elem.h:87 grid_for(n / 4 + 1, 256): four samples per thread"),
    "fmod": (4096, "kernels_elem.h:718 FMOD_TILE = 256 * FMOD_LC = 4096"),
    "hilbwin": (4096, "kernels_firwin.h:39 FWR_TILE = 4096"),
    "mfma1x4": (4096, "stage_fir.h launch_hilbert_mfma: FirMfmaGeom<1, 1>::tile_out(4) = 4 waves * 4 * 16 * 16"),
    "fmt": (1024, "stage_elem2.h:66 items = ns / 4 scalars per thread, 256 threads"),
    "pack": (256, "stage_elem2.h:41 grid_for(ns, 256): one scalar per thread"),
    # FIR forms (stage_fir.h, kernels_fir.h:184 tile_out = nw * nacc * (16 / S) * 16)
    "decfft": (3584, "stage_fir.h launch_decfft_d: wgs of 4 waves x rounds (1) quads of 4 blocks, kernels_firdecfft.h:55 DF_LO = 224 outputs per block"),
    "winshort": (1280, "kernels_firwin2.h:41 TO = 256 * R, R = 5 (stage_fir.h core: launch_win_cplx_m<M, 0, 1, true> = FwcGeom<1, 5, M, 0>), TA = TO"),
    "shortreal": (1024, "stage_fir.h launch_short_real: grid_for((n + 3) / 4, 256): four outputs per thread"),
    "winpair": (2560, "stage_fir.h launch_win_cplx_m: ntiles over 2 * G::TO, TO = 256 * 5"),
    "decimlds50": (121, "stage_fir.h launch_decim_lds: OW = (span_max - M) / D + 1 =(6144 or 6128 - 128) / 50 + 1"),
    "direct": (256, "stage_fir.h launch_direct: grid_for(n_out, 256)"),
    "mfmacc": (4096, "stage_fir.h dispatch_mfma_cc: launch_mfma_cc<2, 4>: FirMfmaGeom<1, 2>::tile_out(4)"),
    "mfma2d1": (4096, "stage_fir.h dispatch_mfma: launch_mfma<2, 1, 8>: tile_out(8) = 4 * 8 * 8 * 16"),
    "mfma1d1": (8192, "stage_fir.h dispatch_mfma: launch_mfma<1, 1, 8>: tile_out(8) = 4 * 8 * 16 * 16"),
    "mfma2d5": (1024, "stage_fir.h dispatch_mfma: launch_mfma<2, 5, 2>: tile_out(2) = 4 * 2 * 8 * 16"),
    "iir": (4096, "kernels_iir.h:24 IIR_TILE = 256 * IIR_LC"),
    "agc": (2048, "kernels_agc.h:22 AGC_TILE = 256 * AGC_LC"),
}


def T(form):
    return TILES[form][0]


class TorchMemory:
    """device allocations through torch; an address is data_ptr() + byte offset"""

    def __init__(self):
        import torch
        self.torch = torch

    def alloc(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda")

    def write(self, h, data):
        h.copy_(self.torch.from_numpy(np.ascontiguousarray(data)))

    def read(self, h):
        return h.cpu().numpy()

    def addr(self, h, off):
        return h.data_ptr() + off

    def sync(self):
        self.torch.cuda.synchronize()
        _lib.check(_lib.load().lrhip_synchronize(), "synchronize")


class RawStage:
    """a stage made by an lrhip_*_create call that no Python block wraps"""

    def __init__(self, ptr, what):
        self._stage = _lib.check_ptr(ptr, what)

    def stage_handle(self):
        return self._stage

    def max_output(self, n):
        return _lib.load().lrhip_stage_max_output(self._stage, n)

    def reset(self):
        _lib.check(_lib.load().lrhip_stage_reset(self._stage), "reset")

    def __del__(self):
        try:
            _lib.load().lrhip_stage_destroy(self._stage)
        except Exception:
            pass


def device_call(obj, ins, n, outs, cap):
    """process_device of a block, chain or composite; lrhip_stage_execute2_device for two inputs"""
    if len(ins) == 2:
        return _lib.check(_lib.load().lrhip_stage_execute2_device(obj.stage_handle(), ins[0], ins[1], n, outs[0], cap), "execute2_device")
    if hasattr(obj, "process_device"):
        return obj.process_device(ins[0], n, outs[0], cap)
    return _lib.check(_lib.load().lrhip_stage_execute_device(obj.stage_handle(), ins[0], n, outs[0], cap), "execute_device")


def make(cls, args, in_types, rate=RATE, **attrs):
    blk = cls(*args)
    blk.rate = rate
    for k, v in attrs.items():
        setattr(blk, k, v)
    blk.differentiate(list(in_types))
    blk.initialize()
    return blk


def reused(obj):
    """a factory that hands out one object, reset (the filters whose tables take a while to build)"""
    def factory():
        obj.reset()
        return obj
    return factory


def rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


def rand_r(rng, n):
    return rng.uniform(-1, 1, n).astype(np.float32)


def rand(rng, n, cplx):
    return rand_c(rng, n) if cplx else rand_r(rng, n)


def tp(cplx):
    return types.ComplexFloat32 if cplx else types.Float32


def len_pairs(t, vec16=False):
    """two consecutive calls; over the pairs every n of {1, 3, 2T + 1, 3T - 1, 3T} is sent, the small ones as first and as second call"""
    pairs = [(2 * t + 1, 3), (1, 3 * t - 1), (3, 3 * t), (3 * t, 1)]
    if vec16:
        pairs.append((2 * t + 2, 2 * t + 3))
    return pairs


def chunks(proc, xs, pair):
    """a stateful oracle over the calls of `pair`"""
    out, a = [], 0
    for n in pair:
        out.append(np.asarray(proc(*[x[a:a + n] for x in xs])))
        a += n
    return out


def checker(want, tol):
    """(f): bit equality (tol None), max |got - want| < tol, or tol(got, want, call)"""
    def check(c, got):
        w = want[c]
        assert len(got) == len(w), (c, len(got), len(w))
        if tol is None and got.dtype.kind == "V":
            assert got.tobytes() == w.tobytes(), c
        elif tol is None:
            assert np.array_equal(got, w), (c, np.flatnonzero(got != w)[:4])
        elif callable(tol):
            tol(got, w, c)
        elif len(w):
            err = G.max_abs_err(got, w)
            assert err < tol, (c, err, tol, int(np.argmax(np.abs(got.astype(np.complex128) - w.astype(np.complex128)))))
    return check


def guarded(factory, inputs, want, tol, pairs, in_offs=(0, 1), out_offs=(0, 1), **kw):
    """every call-length pair at every pointer offset; want(pair) -> the expected outputs of the two calls"""
    mem = TorchMemory()
    for pair in pairs:
        w = want(pair) if want is not None else None
        for io in in_offs:
            for oo in out_offs:
                try:
                    GD.run_guarded(factory, inputs, list(pair), io, oo, mem=mem, call=device_call, max_output=lambda obj, n: obj.max_output(n),
                                   check=checker(w, tol) if w is not None else None, **kw)
                except AssertionError as e:
                    raise AssertionError("lens %s, input offset %s, output offset %s: %s" % (pair, io, oo, e)) from None
                except (RuntimeError, _lib.LrhipError) as e:
                    if any(w in str(e) for w in ("illegal memory access", "launch failure", "hipErrorIllegal")):
                        pytest.exit("GPU fault at lens %s, offsets %s / %s: %s - nothing more is started on this device" % (pair, io, oo, e), 3)
                    raise


def total(pairs):
    return max(sum(p) for p in pairs)


# ===================================================================================================== element-wise stages
def _f64c(x):
    return x.astype(np.complex128)


UNARY = {
    # name: (block, args, complex in, out dtype, form, float64 definition, golden spec (None: bit equality))
    "complexmagnitude": ("ComplexMagnitudeBlock", [], True, np.float32, "unary4", lambda x: np.abs(_f64c(x)), "complexmagnitude_spec"),
    "complexphase": ("ComplexPhaseBlock", [], True, np.float32, "unary4", lambda x: np.angle(_f64c(x)), "complexphase_spec"),
    "complextoreal": ("ComplexToRealBlock", [], True, np.float32, "unary4", lambda x: x.real, None),
    "complextoimag": ("ComplexToImagBlock", [], True, np.float32, "unary4", lambda x: x.imag, None),
    "complexconjugate": ("ComplexConjugateBlock", [], True, np.complex64, "unary2", lambda x: np.conj(x), None),
    "realtocomplex": ("RealToComplexBlock", [], False, np.complex64, "unary2", lambda x: x.astype(np.complex64), None),
    "absolutevalue": ("AbsoluteValueBlock", [], False, np.float32, "unary4", lambda x: np.abs(x), None),
    "addconstant-real": ("AddConstantBlock", [0.375], False, np.float32, "unary4", lambda x: x.astype(np.float64) + 0.375, "addconstant_spec"),
    "addconstant-complex-by-real": ("AddConstantBlock", [0.375], True, np.complex64, "unary2", lambda x: _f64c(x) + 0.375, "addconstant_spec"),
    "addconstant-complex": ("AddConstantBlock", [0.375 - 1.5j], True, np.complex64, "unary2", lambda x: _f64c(x) + (0.375 - 1.5j), "addconstant_spec"),
}


@pytest.mark.parametrize("name", list(UNARY))
def test_unary(name):
    """the ten operations of unary_vec_kernel / unary_kernel (an offset pointer takes the one-sample kernel)"""
    cls, args, cplx, out_dtype, form, define, spec = UNARY[name]
    pairs = len_pairs(T(form), vec16=True)
    x = rand(np.random.default_rng(len(name)), total(pairs), cplx)
    tol = G.load(spec)["epsilon"] if spec else None
    guarded(lambda: make(getattr(lr, cls), args, [tp(cplx)]), [x], lambda pair: chunks(lambda v: define(v).astype(out_dtype), [x], pair), tol, pairs,
            out_dtype=out_dtype)


BINARY = {
    "multiply": ("MultiplyBlock", lambda a, b: a.astype(np.complex128 if a.dtype.kind == "c" else np.float64) * b, "multiply_spec"),
    "multiplyconjugate": ("MultiplyConjugateBlock", None, None),
    "add": ("AddBlock", lambda a, b: a.astype(np.complex128 if a.dtype.kind == "c" else np.float64) + b, "add_spec"),
    "subtract": ("SubtractBlock", lambda a, b: a.astype(np.complex128 if a.dtype.kind == "c" else np.float64) - b, "subtract_spec"),
}


@pytest.mark.parametrize("name,cplx", [(n, c) for n in BINARY for c in (True, False) if c or n != "multiplyconjugate"])      # (its signature is ComplexFloat32 only)
def test_binary(name, cplx):
    """binary_vec4_kernel on the whole float4s, the scalar kernels on the up to three floats behind them and on offset pointers"""
    cls, define, spec = BINARY[name]
    pairs = len_pairs(T("vec4c" if cplx else "vec4r"), vec16=True)
    rng = np.random.default_rng(7 + cplx)
    a, b = rand(rng, total(pairs), cplx), rand(rng, total(pairs), cplx)
    dt = a.dtype
    if define is None:
        want, tol = (lambda pair: chunks(lambda u, v: O.multiply_conjugate(u, v), [a, b], pair)), None          # same single-rounding arithmetic
    else:
        want, tol = (lambda pair: chunks(lambda u, v: define(u, v).astype(dt), [a, b], pair)), G.load(spec)["epsilon"]
    guarded(lambda: make(getattr(lr, cls), [], [tp(cplx), tp(cplx)]), [a, b], want, tol, pairs, out_dtype=dt)


@pytest.mark.parametrize("mode", ["real-real", "real-complex", "complex-complex"])
def test_multiplyconstant(mode):
    cplx = mode != "real-real"
    const = (0.75 - 0.5j) if mode == "complex-complex" else 0.75
    pairs = len_pairs(T("vec4c" if cplx else "vec4r"), vec16=True)
    x = rand(np.random.default_rng(11), total(pairs), cplx)
    define = lambda v: (v.astype(np.complex128 if cplx else np.float64) * const).astype(x.dtype)  # noqa: E731
    guarded(lambda: make(lr.MultiplyConstantBlock, [const], [tp(cplx)]), [x], lambda pair: chunks(define, [x], pair),
            G.load("multiplyconstant_spec")["epsilon"], pairs, out_dtype=x.dtype)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("L", [3, 4, 5])
def test_upsampler(L, cplx):
    """upsample_vec_kernel: UPS_U 16-byte stores per thread, the samples behind the last whole store on the thread after them"""
    t = -(-T("upsc" if cplx else "upsr") // L)
    pairs = len_pairs(t, vec16=True)
    x = rand(np.random.default_rng(L), total(pairs), cplx)

    def define(v):
        y = np.zeros(len(v) * L, x.dtype)
        y[::L] = v
        return y
    guarded(lambda: make(lr.UpsamplerBlock, [L], [tp(cplx)]), [x], lambda pair: chunks(define, [x], pair), None, pairs, out_dtype=x.dtype)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("factor", [2, 7])
def test_downsampler(factor, cplx):
    pairs = len_pairs(T("one") * factor)
    x = rand(np.random.default_rng(factor), total(pairs), cplx)
    guarded(lambda: make(lr.DownsamplerBlock, [factor], [tp(cplx)]), [x], lambda pair: chunks(O.Downsampler(factor, cplx).process, [x], pair), None, pairs,
            out_dtype=x.dtype)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("D", [3, 4, 1028])
def test_delay(D, cplx):
    """D = 4 and 1028 with whole float4s of input take delay_vec_kernel (the pairs of even lengths), everything else delay_kernel"""
    t = T("delay4") // (2 if cplx else 1)
    pairs = len_pairs(t) + [(2 * t + 4, 3 * t), (3 * t - 4, 2 * t + 8)]
    x = rand(np.random.default_rng(D), total(pairs), cplx)

    def want(pair):
        s = np.concatenate([np.zeros(D, x.dtype), x])
        return [s[:pair[0]], s[pair[0]:pair[0] + pair[1]]]
    guarded(lambda: make(lr.DelayBlock, [D], [tp(cplx)]), [x], want, None, pairs, out_dtype=x.dtype)


def test_floattocomplex():
    pairs = len_pairs(T("f2c"), vec16=True)
    rng = np.random.default_rng(21)
    a, b = rand_r(rng, total(pairs)), rand_r(rng, total(pairs))
    guarded(lambda: make(lr.FloatToComplexBlock, [], [types.Float32, types.Float32]), [a, b],
            lambda pair: chunks(lambda u, v: (u + 1j * v).astype(np.complex64), [a, b], pair), None, pairs, out_dtype=np.complex64)


def test_complextofloat():
    """ComplexToFloatBlock is two device passes, ComplexToReal and ComplexToImag (test_unary): here through its own sub-blocks"""
    pairs = len_pairs(T("unary4"), vec16=True)
    x = rand_c(np.random.default_rng(22), total(pairs))
    for port, part in ((0, np.real), (1, np.imag)):
        guarded(lambda: make(lr.ComplexToFloatBlock, [], [types.ComplexFloat32])._sub_blocks[port], [x],
                lambda pair: chunks(lambda v: part(v).astype(np.float32), [x], pair), None, pairs, out_dtype=np.float32)


def test_frequencytranslator():
    """rotator_kernel<2> (two float4 per thread, the second clamped to the first past the end) and rotator_kernel<1> on offset pointers"""
    pairs = len_pairs(T("rot2"), vec16=True)
    x = rand_c(np.random.default_rng(23), total(pairs))
    offset = -0.7318
    guarded(lambda: make(lr.FrequencyTranslatorBlock, [offset], [types.ComplexFloat32]), [x],
            lambda pair: chunks(O.Rotator(2 * np.pi * offset / RATE, O.MODE_F64).process, [x], pair), 1e-6, pairs, out_dtype=np.complex64)


def test_frequencydiscriminator():
    """output offsets of 0, 1 and 2 floats select fmdiscrim_vec4_kernel, fmdiscrim_kernel and fmdiscrim_vec2_kernel"""
    pairs = len_pairs(T("disc4"), vec16=True)
    x = rand_c(np.random.default_rng(24), total(pairs))
    guarded(lambda: make(lr.FrequencyDiscriminatorBlock, [1.25], [types.ComplexFloat32]), [x],
            lambda pair: chunks(O.FMDiscriminator(1.25).process, [x], pair), 1e-6, pairs, out_offs=(0, 1, 2), out_dtype=np.float32)


def test_frequencymodulator():
    pairs = len_pairs(T("fmod"))
    x = rand_r(np.random.default_rng(25), total(pairs))
    guarded(lambda: make(lr.FrequencyModulatorBlock, [0.2], [types.Float32]), [x], lambda pair: chunks(O.FMModulator(0.2).process, [x], pair), 1e-6, pairs,
            out_dtype=np.complex64)


@pytest.mark.parametrize("ntaps", [65, 129, 33])
def test_hilberttransform(ntaps):
    """65 and 129 taps: hilbert_win_kernel; 33: the Toeplitz kernel with the pair epilogue.  Float64 definition: (input delayed by (M - 1) / 2, FIR of it)"""
    pairs = len_pairs(T("hilbwin" if ntaps != 33 else "mfma1x4"))
    x = rand_r(np.random.default_rng(ntaps), total(pairs))
    blk = make(lr.HilbertTransformBlock, [ntaps], [types.Float32])
    taps = np.asarray(blk.hilbert_taps, np.float32)

    def want(pair):
        im = O.FIR(taps, False, O.MODE_F64).process(x[:sum(pair)])
        re = np.concatenate([np.zeros((ntaps - 1) // 2, np.float32), x])[:sum(pair)]
        y = (re + 1j * im).astype(np.complex64)
        return [y[:pair[0]], y[pair[0]:]]
    guarded(reused(blk), [x], want, G.load("hilberttransform_spec")["epsilon"], pairs, in_offs=(0, 1, 2, 3), out_dtype=np.complex64)


# ===================================================================================================== record formats
def _records(fmt, cplx, n, seed):
    """n records of the format as a (n,) array of `record size` bytes, made from finite samples (so the float formats hold no NaN)"""
    x = rand(np.random.default_rng(seed), n, cplx)
    raw = O.format_pack(fmt, x)
    rec = O.FORMAT_BYTES[fmt] * (2 if cplx else 1)
    return x, np.frombuffer(bytes(raw), np.dtype((np.void, rec)))


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("fmt", list(O.FORMAT_BYTES))
def test_format_convert(fmt, cplx):
    """format_convert_vec_kernel (four scalars per thread, the tail on a spare one) with the records at offset 0, format_convert_kernel at 1 byte"""
    pairs = len_pairs(T("fmt") // (2 if cplx else 1), vec16=True)
    _, rec = _records(fmt, cplx, total(pairs), 31)
    out_dtype = np.complex64 if cplx else np.float32

    def want(pair):
        return chunks(lambda r: O.format_convert(fmt, np.frombuffer(r.tobytes(), np.uint8), cplx), [rec], pair)
    guarded(lambda: RawStage(_lib.load().lrhip_format_convert_create(fmt.encode(), int(cplx)), "format_convert"), [rec], want, None, pairs,
            in_offs=(0, 1), out_offs=(0, 4), in_kind="raw", out_dtype=out_dtype, offsets_in_bytes=True)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("fmt", list(O.FORMAT_BYTES))
def test_format_pack(fmt, cplx):
    pairs = len_pairs(T("pack") // (2 if cplx else 1))
    x, _ = _records(fmt, cplx, total(pairs), 32)
    rec = np.dtype((np.void, O.FORMAT_BYTES[fmt] * (2 if cplx else 1)))

    def want(pair):
        return chunks(lambda v: np.frombuffer(bytes(O.format_pack(fmt, v)), rec), [x], pair)
    guarded(lambda: RawStage(_lib.load().lrhip_format_pack_create(fmt.encode(), int(cplx)), "format_pack"), [x], want, None, pairs,
            in_offs=(0,), out_offs=(0, 1), out_dtype=rec, offsets_in_bytes=True)


# ===================================================================================================== FIR, one case per FirForm
def _lowpass(ntaps, cutoff):
    return O.firwin_lowpass(ntaps, cutoff).astype(np.float32)


def _ctaps(rng, ntaps):
    return (rand_c(rng, ntaps) / ntaps).astype(np.complex64)


# name: (taps, ComplexFloat32 stream, decimation, use_fft, form, input offsets in floats, bar).  Every shape is a row "bounds: <name>" of
# tools/host_fir_form_check.hip.  On a ComplexFloat32 stream an offset of 1 or 3 floats is not sample-aligned: fir_form() then names the direct kernel
# for these plain filters (the polyphase-FFT form goes down the cascade to it), which is what the odd offsets of those cases run.
FIR_NAMES = ["decfft", "winshort", "winshortc", "shortreal", "winpair", "decimlds1", "decimlds2", "direct", "mfmacc", "persistent-cf32", "persistent-f32", "persistent-cf32-d5", "generic-cf32", "generic-f32"]


@functools.lru_cache(maxsize=None)
def fir_forms():
    _R = np.random.default_rng(1234)
    return {
        "decfft": (_lowpass(128, 0.25), True, 4, "fast", "decfft", (0, 1, 2, 3), 1e-6),
        "winshort": (rand_r(_R, 16) / 16, True, 1, False, "winshort", (0, 2), None),
        "winshortc": (_ctaps(_R, 16), True, 1, False, "winshort", (0, 2), None),
        "shortreal": (rand_r(_R, 16) / 16, False, 1, False, "shortreal", (0, 1, 2, 3), None),
        "winpair": (_lowpass(136, 0.2), False, 5, False, "winpair", (0, 1, 2, 3), None),
        "decimlds1": (_lowpass(128, 0.02), False, 50, False, "decimlds50", (0, 1, 2, 3), None),
        "decimlds2": (_lowpass(128, 0.02), True, 50, False, "decimlds50", (0, 2), None),
        "direct": (_lowpass(128, 0.136), True, 1, False, "direct", (1, 3), None),
        "mfmacc": (_ctaps(_R, 64), True, 1, False, "mfmacc", (0, 1, 2, 3), None),
        "persistent-cf32": (_lowpass(128, 0.136), True, 1, False, "mfma2d1", (0, 2), None),
        "persistent-f32": (_lowpass(128, 0.136), False, 1, False, "mfma1d1", (0, 1, 2, 3), None),
        "persistent-cf32-d5": (_lowpass(128, 0.2), True, 5, False, "mfma2d5", (0, 1, 2, 3), None),
        "generic-cf32": (_lowpass(124, 0.136), True, 1, False, "mfma2d1", (0, 1, 2, 3), None),
        "generic-f32": (_lowpass(132, 0.136), False, 1, False, "mfma1d1", (0, 1, 2, 3), None),
    }


def _fir_oracle(taps, cplx, D, mode):
    fir = O.FIR(taps, cplx, mode)
    return fir.process if D == 1 else O.Chain([fir, O.Downsampler(D, cplx)]).process


@pytest.mark.parametrize("name", FIR_NAMES)
def test_fir_form(name):
    """every FirForm that fir_form() returns without an environment knob (WinReal and WinCplx are opt-in).  Direct form: the bits of the fmaf chain in
    the reference's tap order (test_fir_real_taps_bit_exact_vs_fma_oracle and its neighbours); the polyphase-FFT form: 1e-6 against float64"""
    taps, cplx, D, use_fft, form, offs, tol = fir_forms()[name]
    pairs = len_pairs(T(form) * D)
    x = rand(np.random.default_rng(len(name)), total(pairs), cplx)
    blk = make(lr.FIRFilterBlock, [taps, use_fft], [tp(cplx)], decimation=D)
    mode = O.MODE_FMA if tol is None else O.MODE_F64
    guarded(reused(blk), [x], lambda pair: chunks(_fir_oracle(taps, cplx, D, mode), [x], pair), tol, pairs, in_offs=[4 * o for o in offs],
            out_offs=(0, 8 if cplx else 4), out_dtype=x.dtype, offsets_in_bytes=True)


def _chain_blocks(rate=1102500.0, decim=5, disc=True):
    bl = [make(lr.FrequencyTranslatorBlock, [-250e3], [types.ComplexFloat32], rate=rate),
          make(lr.LowpassFilterBlock, [128, 100e3], [types.ComplexFloat32], rate=rate)]
    if decim > 1:
        bl.append(make(lr.DownsamplerBlock, [decim], [types.ComplexFloat32], rate=rate))
    if disc:
        bl.append(make(lr.FrequencyDiscriminatorBlock, [1.25], [types.ComplexFloat32], rate=rate))
    return bl


@pytest.mark.parametrize("disc", [False, True])
def test_fused_rotator_on_an_unaligned_pointer_is_an_error(disc):
    """a fused rotator / discriminator on an input pointer that is not sample-aligned: the documented outcome is an error return
    (stage_fir.h launch_mfma_ks), and nothing at all is written"""
    import torch
    blocks = _chain_blocks(disc=disc)
    chain = lr.Chain(blocks)
    n = 5 * T("mfma2d5") + 7
    x = rand_c(np.random.default_rng(3), n)
    size = 2 * GD.G + 8 * n + 16
    img = GD._input_image(size, GD.G + 4, np.frombuffer(x.tobytes(), np.uint8), "float", True, None)
    xin = torch.from_numpy(img.copy()).cuda()
    out = torch.from_numpy(GD.sentinel_fill(size).copy()).cuda()
    torch.cuda.synchronize()
    with pytest.raises(_lib.LrhipError, match="sample-aligned"):
        chain.process_device(xin.data_ptr() + GD.G + 4, n, out.data_ptr() + GD.G, chain.max_output(n))
    _lib.load().lrhip_synchronize()
    GD.check_after(out.cpu().numpy(), GD.G, 0)
    GD.check_before(out.cpu().numpy(), GD.G)
    GD.check_input_untouched(img, xin.cpu().numpy(), GD.G + 4)


# ===================================================================================================== FIR, one case per FirFftForm
def _fft_tile(ntaps, cplx):
    """outputs per block of the form fir_fft_form() names for a small launch (stage_fir.h launch_fft): the 1024-point kernel advances by
    1024 - 64 ceil((M - 1) / 64) (:482), the 4096-point kernels by 4096 - V (:357, :374), the 64 x 64 form at an overlap of 2 048 by 2 048 (:392); a Float32
    stream rides two blocks per transform (:379, :484)"""
    if ntaps <= 512:
        lf = 1024 - (ntaps - 1 + 63) // 64 * 64
    elif ntaps <= 1281:
        lf = 4096 - max(768, (ntaps - 1 + 255) // 256 * 256)
    else:
        lf = 2048
    return lf if cplx else 2 * lf


FFT_TAPS = [128, 512, 513, 1281, 1282, 2049, 2050, 4097, 4098]


def _norm_taps(rng, ntaps, cplx_taps):
    taps = rand_c(rng, ntaps) if cplx_taps else rand_r(rng, ntaps)
    return (taps / np.sum(np.abs(taps))).astype(taps.dtype)           # like the reference's normalize()


@pytest.mark.parametrize("ntaps", FFT_TAPS)
@pytest.mark.parametrize("stream", ["cf32-real", "cf32-complex", "f32-real"])
def test_fir_fft_form(stream, ntaps):
    """use_fft = "fast" across the partition boundaries 512 / 513, 1 281 / 1 282, 2 049 / 2 050, 4 097 / 4 098 (4 098: two launches, the second adds to y):
    Pass1024, Wg4k (ComplexFloat32) / Wave64 (Float32), Long64.  The bar of test_fir_fft_arithmetic_fast_mode: 1e-6 against float64"""
    cplx, cplx_taps = stream.startswith("cf32"), stream.endswith("complex")
    rng = np.random.default_rng(ntaps + 7 * cplx + 13 * cplx_taps)
    taps = _norm_taps(rng, ntaps, cplx_taps)
    pairs = len_pairs(_fft_tile(ntaps, cplx))
    x = rand(rng, total(pairs), cplx)
    blk = make(lr.FIRFilterBlock, [taps, "fast"], [tp(cplx)])
    guarded(reused(blk), [x], lambda pair: chunks(O.FIR(taps, cplx, O.MODE_F64).process, [x], pair), 1e-6, pairs, in_offs=(0, 4, 8, 12),
            out_offs=(0, 8 if cplx else 4), out_dtype=x.dtype, offsets_in_bytes=True)


@pytest.mark.parametrize("which", ["wave64", "pols"])
def test_fir_fft_large(which):
    """the two forms only a large launch reaches, at the smallest n_out for which fir_fft_form() names them on this chip: Wave64 on a ComplexFloat32
    stream from 20 blocks of 4 096 - 1 280 outputs per CU, Pols on a Float32 stream of 768 taps from one transform more than a round of 8 waves per
    CU.  Guards, holes, input and the hostile / finite comparison are checked on the device; the first outputs and the last block of each call
    come back for the oracle."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if which == "wave64":
        cplx, ntaps, lf = True, 1281, 4096 - 1280
        n1 = (20 * cus - 1) * lf + 1
    else:
        cplx, ntaps, lf = False, 768, 2 * (4096 - 768)
        n1 = (8 * cus) * lf + 1
    rng = np.random.default_rng(ntaps)
    taps = _norm_taps(rng, ntaps, False)
    lens = [n1, 3]
    x = rand(rng, sum(lens), cplx)
    es = x.dtype.itemsize
    sent = int(np.array(GD.SENT).view(np.int32))
    blk = make(lr.FIRFilterBlock, [taps, "fast"], [tp(cplx)])
    L = _lib.load()
    slab = lf + 64
    for off in (0, 1):
        outs = {}
        for hostile in (True, False):
            blk.reset()
            gw, ow = GD.G_WORDS, off * es // 4
            xin = (torch.full((2 * gw + ow + n1 * es // 4,), sent, dtype=torch.int32, device="cuda") if hostile
                   else torch.rand(2 * gw + ow + n1 * es // 4, device="cuda").view(torch.int32))
            out = torch.empty(2 * gw + ow + n1 * es // 4, dtype=torch.int32, device="cuda")
            pos, got = 0, []
            for c, n in enumerate(lens):
                nw = n * es // 4
                xin[gw + ow:gw + ow + nw] = torch.from_numpy(x[pos:pos + n].view(np.int32)).cuda()
                if hostile:
                    xin[gw + ow + nw:] = sent
                before = xin.clone()
                out.fill_(sent)
                torch.cuda.synchronize()
                count = blk.process_device(xin.data_ptr() + 4 * (gw + ow), n, out.data_ptr() + 4 * (gw + ow), blk.max_output(n))
                L.lrhip_synchronize()
                assert count == n
                tag = (which, off, hostile, c)
                bad = (out[:gw + ow] != sent).nonzero()
                assert bad.numel() == 0, ("(a) write before out", tag, int(bad[0]) - gw - ow)
                bad = (out[gw + ow + nw:] != sent).nonzero()
                assert bad.numel() == 0, ("(b) write at or after the count", tag, int(bad[0]) + nw)
                y = out[gw + ow:gw + ow + nw]
                bad = (y == sent).nonzero()
                assert bad.numel() == 0, ("(c) unwritten word", tag, int(bad[0]))
                assert bool(torch.isfinite(y.view(torch.float32)).all()), ("(c) non-finite output", tag)
                assert torch.equal(before, xin), ("(d) input modified", tag)
                got.append(y.clone())
                # (f) the first outputs and the last block of the call against float64
                for a, b in ((0, min(n, slab)), (max(0, n - slab), n)):
                    lo = max(0, pos + a - (ntaps - 1))                   # the taps' reach in front of the slab
                    want = O.FIR(taps, cplx, O.MODE_F64).process(x[lo:pos + b])[pos + a - lo:]
                    have = y[a * es // 4:b * es // 4].cpu().numpy().view(x.dtype)
                    assert G.max_abs_err(have, want) < 1e-6, ("(f)", tag, a, b)
                pos += n
            outs[hostile] = got
        for c in range(len(lens)):
            assert torch.equal(outs[True][c], outs[False][c]), ("(e) the output depends on words outside the input", which, off, c)


# ===================================================================================================== IIR
def _poles(order, radius):
    ang = np.linspace(0.15, 1.2, order // 2)
    poles = list(radius * np.exp(1j * ang)) + list(radius * np.exp(-1j * ang)) + ([0.5] if order % 2 else [])
    return (np.real(np.poly([-1.0] * 3)) * 0.01).astype(np.float32), np.real(np.poly(poles)).astype(np.float32)


IIR_NAMES = ["order1-single", "order1-threepass", "golden0", "golden1"] + ["order%d-%s" % (o, p) for o in (2, 4, 5, 8) for p in ("single", "threepass")]


@functools.lru_cache(maxsize=None)
def iir_cases():
    cases = {}
    # order 1 as test_iir_single_launch_and_three_pass_paths_vs_oracle has it: pole 0.94 (single launch) and 0.99993 (three passes), 2e-6
    for name, (cutoff, rate) in (("order1-single", (2122.0, 220500.0)), ("order1-threepass", (0.5, 48000.0))):
        cases[name] = tuple(np.asarray(v, np.float32) for v in O.singlepole_lowpass_taps(cutoff, rate)) + (2e-6,)
    # orders 2 and 4: the golden filters of test_iir_second_and_fourth_order_scan_large, 2e-6
    for i, vec in enumerate(G.load("iirfilter_spec")["vectors"][:2]):
        b, a = vec["args"]
        cases["golden%d" % i] = (np.asarray(b, np.float32), np.asarray(a, np.float32), 2e-6)
    # orders 2 .. 8 with short-memory poles (radius 0.85: the single-launch kernel) and poles at 0.9995 (three passes), the bar of
    # test_iir_orders_five_to_eight_scan_paths: at most ten times the error of the sequential Float32 recurrence, plus 2e-6 of the scale
    for order in (2, 4, 5, 8):
        for radius, path in ((0.85, "single"), (0.9995, "threepass")):
            cases["order%d-%s" % (order, path)] = _poles(order, radius) + ("yardstick",)
    assert list(cases) == IIR_NAMES
    return cases


def _iir_bar(b, a, cplx, x, bar):
    if bar != "yardstick":
        return bar
    want = O.IIR(b, a, cplx, O.MODE_F64).process(x)
    yard = G.max_abs_err(O.IIR(b, a, cplx, O.MODE_LUA).process(x), want)
    return 10 * yard + 2e-6 * max(1.0, float(np.max(np.abs(want))))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", IIR_NAMES)
def test_iir(name, cplx):
    b, a, bar = iir_cases()[name]
    pairs = len_pairs(T("iir"))
    x = rand(np.random.default_rng(len(name) + cplx), total(pairs), cplx)
    tol = _iir_bar(b, a, cplx, x, bar)
    guarded(lambda: make(lr.IIRFilterBlock, [b, a], [tp(cplx)]), [x], lambda pair: chunks(O.IIR(b, a, cplx, O.MODE_F64).process, [x], pair), tol, pairs,
            out_dtype=x.dtype)


# ===================================================================================================== gain and squelch
def _levels(rng, n, cplx, low, high, step):
    """full-scale noise whose level alternates every `step` samples between a draw from the dB range `low` and one from `high`"""
    k = n // step + 1
    db = np.where(np.arange(k) % 2 == 0, rng.uniform(*low, k), rng.uniform(*high, k))
    level = 10 ** (np.repeat(db, step)[:n] / 20)
    return (rand(rng, n, cplx) * level.astype(np.float32)).astype(np.complex64 if cplx else np.float32)


@pytest.mark.parametrize("cplx", [True, False])
def test_agc(cplx):
    """the bar of test_agc_parallel_scans_vs_sequential_oracle: 2e-5 relative to max(|want|, 1e-6), levels stepping across the threshold"""
    rate = 48000.0
    pairs = len_pairs(T("agc"))
    x = _levels(np.random.default_rng(55 + cplx), total(pairs), cplx, (-90, -70), (-50, -20), 700)

    def bar(got, want, c):
        assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-6)) < 2e-5, c
    guarded(lambda: make(lr.AGCBlock, ["fast", -35, -60], [tp(cplx)], rate=rate), [x],
            lambda pair: chunks(O.AGC("fast", -35, -60, rate, cplx).process, [x], pair), bar, pairs, out_dtype=x.dtype)


@pytest.mark.parametrize("cplx", [True, False])
def test_powersquelch(cplx):
    """the float64 recurrence of test_golden_powersquelch_and_large and its bar: a threshold crossing may land one sample apart (at most two
    samples differ), everything else is the input or zero, bit for bit"""
    rate = 48000.0
    pairs = len_pairs(T("agc"))
    x = _levels(np.random.default_rng(66 + cplx), total(pairs), cplx, (-80, -55), (-35, -20), 500)

    def want(pair):
        alpha, p, thr = 1 / (1 + 0.001 * rate), 0.0, 10 ** (-45 / 10)
        e = (x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2) if cplx else x.astype(np.float64) ** 2
        w = np.empty_like(x[:sum(pair)])
        for i in range(sum(pair)):
            p = (1 - alpha) * p + alpha * e[i]
            w[i] = x[i] if p >= thr else 0
        assert 0 < np.count_nonzero(w) < len(w)
        return [w[:pair[0]], w[pair[0]:]]

    def bar(got, w, c):
        assert np.count_nonzero(got != w) <= 2, c
    guarded(lambda: make(lr.PowerSquelchBlock, [-45], [tp(cplx)], rate=rate), [x], want, bar, pairs, out_dtype=x.dtype)


# ===================================================================================================== spectrum
def _window(N):
    win = np.asarray(lr.window_utils.window(N, "hamming", True), np.float32)
    return win, 44100.0 * float(np.sum(win.astype(np.float64) ** 2))


@pytest.mark.parametrize("N", [8, 1024, 4096])
@pytest.mark.parametrize("kind", ["dft-complex", "dft-real", "idft-complex", "idft-real", "psd", "psd-log"])
def test_spectrum(kind, N):
    """DFT, IDFT and PSD frames, one frame and three frames per call; the bars of test_dft_idft_psd_other_frame_sizes_vs_oracle and test_psd_many_frames_vs_oracle"""
    L = _lib.load()
    rng = np.random.default_rng(N + len(kind))
    pairs = [(N, 3 * N), (3 * N, N)]
    real = kind.endswith("real")
    if kind.startswith("idft"):
        t = rand(rng, 4 * N, not real)
        x = np.concatenate([O.dft(t[f * N:(f + 1) * N]) for f in range(4)]).astype(np.complex64)
        out_dtype = np.float32 if real else np.complex64
        factory = lambda: RawStage(L.lrhip_dft_create(N, 1, int(real)), kind)  # noqa: E731
        frame, bar = (lambda v: O.idft(v, not real)), (lambda got, w: G.max_abs_err(got, w) < 2e-6)
    elif kind.startswith("dft"):
        x, out_dtype = rand(rng, 4 * N, not real), np.complex64
        factory = lambda: RawStage(L.lrhip_dft_create(N, 0, int(real)), kind)  # noqa: E731
        frame, bar = O.dft, (lambda got, w: G.max_abs_err(got, w) / np.max(np.abs(w)) < 2e-6)
    else:
        log = kind == "psd-log"
        x, out_dtype = rand_c(rng, 4 * N), np.float32
        win, scale = _window(N)
        factory = lambda: RawStage(L.lrhip_psd_create(N, win.ctypes.data_as(C.POINTER(C.c_float)), scale, int(log), 1, 0), kind)  # noqa: E731
        frame = lambda v: O.psd(v, "hamming", 44100.0, log)  # noqa: E731
        bar = (lambda got, w: G.max_abs_err(got, w) < 1e-2) if log else (lambda got, w: np.max(np.abs(got - w)) / np.max(w) < 1e-5)

    def want(pair):
        return chunks(lambda v: np.concatenate([frame(v[f * N:(f + 1) * N]) for f in range(len(v) // N)]), [x], pair)

    def check(got, w, c):
        for f in range(len(w) // N):
            assert bar(got[f * N:(f + 1) * N], np.asarray(w[f * N:(f + 1) * N])), (c, f)
    guarded(factory, [x], want, check, pairs, out_dtype=out_dtype)


@pytest.mark.parametrize("cplx", [True, False])
def test_welch_reads_only_its_input(cplx):
    """WelchSpectrum writes no stream output: the input allocation is untouched (d) and lrhip_welch_read gives the same bytes with hostile and with
    finite words next to the input (e); frames overlap by half, so the second call starts on carried samples"""
    import torch
    N = 256
    lens = [5 * N + 3, 3 * N - 1]
    x = rand(np.random.default_rng(90 + cplx), sum(lens), cplx)
    es = x.dtype.itemsize
    reads = {}
    for off in (0, 1):
        for hostile in (True, False):
            w = lr.spectrum_utils.WelchSpectrum(tp(cplx), N, "hamming", 44100.0, 0.5)
            size = 2 * GD.G + (off + max(lens)) * es
            got, pos = [], 0
            for n in lens:
                img = GD._input_image(size, GD.G + off * es, np.frombuffer(x[pos:pos + n].tobytes(), np.uint8), "float", hostile, np.random.default_rng(5))
                xin = torch.from_numpy(img.copy()).cuda()
                torch.cuda.synchronize()
                w.process_device(xin.data_ptr() + GD.G + off * es, n)
                _lib.load().lrhip_synchronize()
                GD.check_input_untouched(img, xin.cpu().numpy(), GD.G + off * es)
                avg = w.average(reset=False)
                assert avg is not None and np.isfinite(avg).all()
                got.append(avg.copy())
                pos += n
            reads[hostile] = got
        GD.check_same([g.view(np.uint8) for g in reads[True]], [g.view(np.uint8) for g in reads[False]])


# ===================================================================================================== counted stages
# The returned count is below the capacity: check (b) covers the words between the two.  T is in INPUT samples here.
from tests.helpers import ax25_model as AX      # noqa: E402
from tests.helpers import digital_model as dm      # noqa: E402
from tests.helpers import ert_framer_model as EF      # noqa: E402
from tests.helpers import ert_model as em      # noqa: E402
from tests.helpers import ert_signals as es      # noqa: E402
from tests.helpers import modulator_model as mm      # noqa: E402
from tests.helpers import phasecorr_model as pcm      # noqa: E402
from tests.helpers import pll_model as plm      # noqa: E402
from tests.helpers import pocsag_model as PG      # noqa: E402
from tests.helpers import rds_model as rdm      # noqa: E402
from tests.helpers import varicode_model as vm      # noqa: E402

TILES.update({
    "dg": (4096, "kernels_digital.h:30 DG_TILE = 256 * DG_LC input samples per workgroup"),
    "ps": (1024, "kernels_bitscan.h:15 PS_TILE = 1024 input samples per workgroup"),
    "pc": (2048, "kernels_phasecorr.h:26 PC_TILE = 256 * PC_LC"),
    "pll": (4096, "stage_pll.h:53 one segment per lane, 64 lanes per workgroup, segments of PLL_MIN_SEGMENT = 64 samples (pll_plan.h:43) with :segment=64"),
    "mod": (4096, "stage_modulator.h:43 grid_for(nitems + 1, 256 * MOD_U), MOD_U = 4 stores of 16 bytes: 4096 Float32 / 2048 ComplexFloat32 outputs"),
})


def symbols(n, P, seed):
    """finite baseband: +-1 symbols of P samples with noise and samples equal to the threshold"""
    rng = np.random.default_rng(seed)
    sym = rng.choice([-1.0, 1.0], size=int(n / P) + 2)
    x = (np.repeat(sym, int(np.ceil(P)))[:n] + 0.3 * rng.standard_normal(n)).astype(np.float32)
    x[rng.integers(0, n, n // 50)] = 0.0
    return x


def counted(factory, inputs, model, pairs, out_dtype, same=None, concat=None, whole=None, in_kind="float", **kw):
    """guards per call; the big calls emit some records and fewer than max_output; (f): the calls' outputs against the model's, call by call - or, for the
    stages whose model may hold a record back until more input arrives, the concatenation against the model's output on the whole stream"""
    mem = TorchMemory()
    for pair in pairs:
        for io in (0, 1):
            for oo in (0, 1):
                outs = GD.run_guarded(factory, inputs, list(pair), io, oo, mem=mem, call=device_call, max_output=lambda obj, n: obj.max_output(n),
                                      in_kind=in_kind, out_dtype=out_dtype, out_floats=np.dtype(out_dtype).kind in "fc", **kw)
                caps = factory()
                for n, got in zip(pair, outs):
                    if n >= 2 * min(T("ps"), T("dg")):
                        assert 0 < len(got) < caps.max_output(n), (pair, n, len(got))
                m = model()
                if whole:
                    want = m(*[x[:sum(pair)] for x in inputs])
                    have = concat(outs) if concat else np.concatenate(outs)
                    assert same(have, want) if same else np.array_equal(have, want), (pair, io, oo)
                else:
                    for c, (got, want) in enumerate(zip(outs, chunks(m, inputs, pair))):
                        assert len(got) == len(want) and (same(got, want) if same else got.tobytes() == np.ascontiguousarray(want).tobytes()), (pair, io, oo, c)


@pytest.mark.parametrize("cplx", [True, False])
def test_sampler(cplx):
    pairs = len_pairs(T("dg"))
    rng = np.random.default_rng(41)
    n = total(pairs)
    clock = np.repeat(rng.choice([-1.0, 0.0, 1.0], size=n // 3 + 1), 3)[:n].astype(np.float32)
    data = rand(rng, n, cplx)
    counted(lambda: make(lr.SamplerBlock, [], [tp(cplx), types.Float32]), [data, clock], lambda: dm.SamplerFast().process, pairs, data.dtype)


def test_clocksampler():
    P = 12500 / 1200
    pairs = len_pairs(T("dg"))
    x = symbols(total(pairs), P, 42)
    counted(lambda: make(lr.ClockSamplerBlock, [RATE / P], [types.Float32]), [x], lambda: dm.ClockSamplerModel(P, 0.0).process, pairs, np.float32)


def test_zerocrossingclockrecovery():
    P = 7.999999
    pairs = len_pairs(T("dg"))
    x = symbols(total(pairs), P, 43)
    guarded(lambda: make(lr.ZeroCrossingClockRecoveryBlock, [RATE / P], [types.Float32]), [x],
            lambda pair: chunks(dm.ZcLiteral(P, 0.0).process, [x], pair), None, pairs, out_dtype=np.float32)


def test_slicer_and_differentialdecoder():
    pairs = len_pairs(T("one"))
    rng = np.random.default_rng(44)
    x = rng.standard_normal(total(pairs)).astype(np.float32)
    x[::97] = 0.125
    guarded(lambda: make(lr.SlicerBlock, [0.125], [types.Float32]), [x], lambda pair: chunks(lambda v: dm.slicer(v, 0.125), [x], pair), None, pairs,
            out_dtype=np.uint8, out_floats=False)
    b = rng.integers(0, 256, total(pairs)).astype(np.uint8)
    for inv in (False, True):
        guarded(lambda: make(lr.DifferentialDecoderBlock, [inv], [types.Bit]), [b], lambda pair: chunks(dm.DiffDecModel(inv).process, [b], pair), None, pairs,
                in_kind="bits", out_dtype=np.uint8, out_floats=False)


def test_preamblesampler():
    Tsym, L, N = 5, 16, 48
    pairs = len_pairs(T("ps"))
    n = total(pairs)
    rng = np.random.default_rng(45)
    pre = rng.integers(0, 2, L).astype(np.uint8)
    pre[-1] = 1
    weights = np.array([1, 1, 1, 1, 1, 1, 0, 0, 0, 1], float)            # the finite members of the alphabet
    x = es.alphabet_signal(n, 46, weights / weights.sum())
    at = 3 * Tsym * L
    while at < n - Tsym:
        at = es.plant_frame(x, at, Tsym, pre, N, rng, float(rng.choice([1.0, 0.5]))) + int(rng.choice([1, Tsym, 3 * Tsym * N]))
    counted(lambda: make(lr.PreambleSamplerBlock, [1.0, pre, N], [types.Float32], rate=float(Tsym)), [x],
            lambda: em.PreambleSamplerFast(Tsym, pre, N).process, pairs, np.float32, same=lambda g, w: np.array_equal(g.view(np.uint32), w.view(np.uint32)))


@pytest.mark.parametrize("invert", [False, True])
def test_manchesterdecoder(invert):
    pairs = len_pairs(T("dg"))
    n = total(pairs)
    rng = np.random.default_rng(47 + invert)
    data = rng.integers(0, 2, n // 2 + 1).astype(np.uint8)
    x = np.stack([data, 1 - data], axis=1).reshape(-1)
    pos = np.sort(rng.choice(len(x), size=n // 200, replace=False))
    x = np.insert(x, pos, x[pos])[:n].astype(np.uint8)                    # repeated bits: clock slips
    counted(lambda: make(lr.ManchesterDecoderBlock, [invert], [types.Bit]), [x], lambda: em.ManchesterFast(invert).process, pairs, np.uint8, in_kind="bits")


def test_varicodedecoder():
    pairs = len_pairs(T("dg"))
    rng = np.random.default_rng(48)
    text = rng.choice(np.frombuffer(b"etaoin shrdlu CQ de 0123", np.uint8), 4 * T("dg")).tolist()
    x = vm.encode(text, idle=rng.integers(0, 3, len(text)).tolist())[:total(pairs)].astype(np.uint8)
    assert len(x) == total(pairs)
    counted(lambda: make(lr.VaricodeDecoderBlock, [], [types.Bit]), [x], lambda: vm.VaricodeLiteral().process, pairs, np.uint8, in_kind="bits")


def _planted(n, frame, gap, seed):
    """random bits with frame(rng) -> bits planted every `gap` bits or so"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    at = 17
    while True:
        f = np.asarray(frame(rng), np.uint8)
        if at + len(f) > n:
            break
        bits[at:at + len(f)] = f
        at += len(f) + int(rng.integers(gap // 2, gap))
    return bits


FRAMERS = {
    # name: (block, frame(rng) -> bits, gap, model() -> process(x), same(got, want), concat(parts))
    "rds": ("RDSFramerBlock", lambda rng: rdm.encode_frame([int(w) for w in rng.integers(0, 1 << 16, 4)]), 200,
            lambda: rdm.RDSFramerLiteral().process, lambda g, w: np.array_equal(np.asarray(g).reshape(-1, 4), w), None),
    "scm": ("SCMFramerBlock", lambda rng: EF.random_frame(EF.PROTOCOLS["scm"], rng)[0], 200, lambda: EF.FramerLiteral(EF.PROTOCOLS["scm"]).process,
            EF.same_records, lambda parts: EF.concat(parts, EF.PROTOCOLS["scm"].dtype)),
    "scm+": ("SCMPlusFramerBlock", lambda rng: EF.random_frame(EF.PROTOCOLS["scm+"], rng)[0], 200, lambda: EF.FramerLiteral(EF.PROTOCOLS["scm+"]).process,
             EF.same_records, lambda parts: EF.concat(parts, EF.PROTOCOLS["scm+"].dtype)),
    "idm": ("IDMFramerBlock", lambda rng: EF.random_frame(EF.PROTOCOLS["idm"], rng)[0], 150, lambda: EF.FramerLiteral(EF.PROTOCOLS["idm"]).process,
            EF.same_records, lambda parts: EF.concat(parts, EF.PROTOCOLS["idm"].dtype)),
    "ax25": ("AX25FramerBlock", lambda rng: AX.framed(AX.random_octets(rng, payload_len=int(rng.integers(0, 20)))), 120,
             lambda: AX.FramerLiteral().process, AX.same_records, AX.concat),
    "pocsag": ("POCSAGFramerBlock", lambda rng: np.concatenate([PG.preamble(64), PG.transmission(PG.random_messages(rng, 2, max_words=2))[0]]), 100,
               lambda: PG.FramerLiteral(eager=True).process, PG.same_records, PG.concat),
}


@pytest.mark.parametrize("name", list(FRAMERS))
def test_framer(name):
    """the RDS, SCM, SCM+, IDM, AX.25 and POCSAG framers on planted frames: as in their parity tests the records of all calls together are those of the
    literal model on the whole stream (the POCSAG block is eager where the reference may hold a frame back)"""
    cls, frame, gap, model, same, concat = FRAMERS[name]
    pairs = len_pairs(T("ps"))
    x = _planted(total(pairs), frame, gap, len(name))
    blk = getattr(lr, cls)
    out_dtype = (types.RDSFrameType if name == "rds" else blk._frame_type).dtype
    counted(lambda: make(blk, [], [types.Bit], rate=1200.0), [x], model, pairs, out_dtype, same=same,
            concat=concat or (lambda parts: np.concatenate(parts)), whole=True, in_kind="bits")


# ===================================================================================================== other stateful stages
def _pll_signal(n):
    rng = np.random.default_rng(11)
    return (np.exp(1j * (2 * np.pi * 0.1 * np.arange(n) + 0.3)) + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


@pytest.mark.parametrize("port", ["out", "error"])
def test_pll(port):
    """both output ports, speculated segments of 64 samples; the bar of test_locked_parity_whole_and_ragged: 1e-6 against the sequential model"""
    loop, mult = (0.01, 0.19, 0.21), 3.0
    pairs = len_pairs(T("pll"))
    x = _pll_signal(total(pairs))

    def block():
        blk = lr.blocks.PLLOutBlock(*loop, mult, port)
        blk.rate, blk.op_knobs = 2.0, ":segment=64"
        blk.differentiate([types.ComplexFloat32])
        blk.initialize()
        return blk

    def want(pair):
        out, err, _ = plm.run(x[:sum(pair)], *loop, mult)
        w = out if port == "out" else err
        return [w[:pair[0]], w[pair[0]:]]
    guarded(block, [x], want, 1e-6, pairs, out_dtype=np.complex64 if port == "out" else np.float32)


@pytest.mark.parametrize("N,I", [(50, 32), (4, 1)])
def test_binaryphasecorrector(N, I):
    """the bar of test_window_mean_parity_at_size: within 2.5e-7 |x| of the rotation by the float64 window mean"""
    pairs = len_pairs(T("pc"), vec16=True)
    rng = np.random.default_rng(N)
    x = (rng.standard_normal(total(pairs)) + 1j * rng.standard_normal(total(pairs))).astype(np.complex64)

    def want(pair):
        w = pcm.correct(x[:sum(pair)], N, I, "mean_fast")
        return [w[:pair[0]], w[pair[0]:]]

    def bar_for(pair):
        def bar(got, w, c):
            xs = x[:pair[0]] if c == 0 else x[pair[0]:sum(pair)]
            assert np.all(np.abs(got.astype(np.complex128) - w) <= 2.5e-7 * np.abs(xs.astype(np.complex128)) + 1e-30), c
        return bar
    for pair in pairs:
        guarded(lambda: make(lr.BinaryPhaseCorrectorBlock, [N, I], [types.ComplexFloat32], rate=1000.0), [x], want, bar_for(pair), [pair], out_dtype=np.complex64)


def _modulator(kind, bits, period):
    cls = lr.PulseAmplitudeModulatorBlock if kind == "pam" else lr.QuadratureAmplitudeModulatorBlock
    table = (mm.pam_table if kind == "pam" else mm.qam_table)(1 << bits)
    return make(cls, [1.0, float(period), 1 << bits, {"msb_first": True}], [types.Bit], rate=1.0), table


@pytest.mark.parametrize("kind,bits,period", [("pam", 1, 1), ("pam", 3, 5), ("qam", 2, 1), ("qam", 4, 7)])
def test_modulator(kind, bits, period):
    """mod_map_kernel (period 1) and mod_hold_kernel, 16-byte stores with the tail on a spare thread; an offset output takes mod_scalar_kernel.  Bit for bit
    against the model, as test_random_bits_ragged_chunks"""
    per_out = T("mod") // (2 if kind == "qam" else 1)
    t = -(-per_out * bits // period)
    pairs = len_pairs(t, vec16=True)
    x = mm.random_bits(np.random.default_rng(bits + period), total(pairs))
    _, table = _modulator(kind, bits, period)
    dt = np.float32 if kind == "pam" else np.complex64
    guarded(lambda: _modulator(kind, bits, period)[0], [x], lambda pair: chunks(mm.ModulatorModel(table, period, True).process, [x], pair), None, pairs,
            in_kind="bits", out_dtype=dt)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("kind,bits,period,down", [("qam", 2, 8, False), ("pam", 3, 3, True)])
def test_shaped_modulator(kind, bits, period, down, exact):
    """modulator -> RootRaisedCosineFilter [-> Downsampler] in a chain: the bits of the separate blocks where the chain keeps every block's arithmetic
    (test_shaped_chain_equals_separate_blocks), the direct form's 1e-6 otherwise"""
    def blocks():
        mod, _ = _modulator(kind, bits, period)
        bl = [mod, make(lr.RootRaisedCosineFilterBlock, [129, 0.35, 1.0], [mod.get_output_type()], rate=float(period))]
        if down:
            bl.append(make(lr.DownsamplerBlock, [2], [mod.get_output_type()], rate=float(period)))
        return bl
    t = -(-1024 * bits // period)
    pairs = len_pairs(t)
    x = mm.random_bits(np.random.default_rng(10), total(pairs))

    def want(pair):
        ref = blocks()

        def proc(v):
            for b in ref:
                v = b.process(v)
            return v
        return chunks(proc, [x], pair)
    guarded(lambda: lr.Chain(blocks(), exact=exact), [x], want, None if exact else 1e-6, pairs, in_kind="bits",
            out_dtype=np.float32 if kind == "pam" else np.complex64)


# ===================================================================================================== fused chains
# Chain.process_device, default and LRHIP_CHAIN_EXACT, one chain per planner rule and pass of chain_plan.h.  The reference of (f) is the same blocks run one by
# one (host path, the same call lengths); the bar is bit equality where the chain's parity test asserts it and its tolerance otherwise.
FS = 1102500.0
TILES.update({
    "cascade": (3328, "chain_plan.h:72 three 256-tap filters merge into 766 taps: the 4096-point kernel, 4096 - 768 outputs per block (stage_fir.h launch_fft4k_ng: Lf)"),
    "resample": (1024, "stage_resample.h:71 ntiles = ceil(n / tq) input samples per tile, tq <= 1024"),
    "rx": (25600, "kernels_rx.h:88 RX_BATCH = 5 120 discriminator samples per batch = 25 600 input samples at decimation 5"),
    "tuner5": (5120, "stage_fir.h dispatch_mfma: launch_mfma<2, 5, 2>: 1024 outputs per tile at decimation 5"),
    "tuner50": (6050, "stage_fir.h launch_decim_lds: OW = 121 outputs per tile at decimation 50"),
    "tail": (12800, "stage_fir.h launch_win_cplx_m: pair mode: 2 * 1280 outputs per tile at decimation 5"),
    "pass1024r": (1792, "stage_fir.h launch_fft: Lf = 1024 - 128 = 896, two blocks of a Float32 stream per transform"),
})


def _mk(specs, in_type, rate):
    """[(class, args[, attrs])] -> initialized blocks with the rate and type propagated down the run"""
    out = []
    for spec in specs:
        cls, args = spec[0], spec[1]
        b = make(cls, args, [in_type], rate=rate, **(spec[2] if len(spec) > 2 else {}))
        out.append(b)
        rate, in_type = b.get_rate(), b.get_output_type()
    return out


def _taps_lp(n, cutoff):
    return np.asarray(lr.filter_utils.firwin_lowpass(n, cutoff), np.float32)


CHAINS = {
    # name: (specs, input type, rate, form, bar in default mode, bar in EXACT mode); a bar of None is bit equality
    "fir-cascade": ([(lr.FIRFilterBlock, [_taps_lp(256, 0.2), "fast"]), (lr.FIRFilterBlock, [_taps_lp(256, 0.3), "fast"]),
                     (lr.FIRFilterBlock, [_taps_lp(256, 0.25), "fast"])], types.ComplexFloat32, RATE, "cascade", 1e-6, 1e-6),
    "interpolator-cf32": ([(lr.MultiplyConstantBlock, [3.0]), (lr.UpsamplerBlock, [3]), (lr.LowpassFilterBlock, [128, 1 / 3, 1.0])], types.ComplexFloat32, RATE,
                          "resample", None, None),
    "resampler-f32": ([(lr.MultiplyConstantBlock, [3.0]), (lr.UpsamplerBlock, [3]), (lr.LowpassFilterBlock, [128, 1 / 3, 1.0]), (lr.DownsamplerBlock, [2])],
                      types.Float32, RATE, "resample", None, None),
    "resampler-cf32": ([(lr.MultiplyConstantBlock, [4.0]), (lr.UpsamplerBlock, [4]), (lr.LowpassFilterBlock, [128, 1 / 5, 1.0]), (lr.DownsamplerBlock, [5])],
                       types.ComplexFloat32, RATE, "resample", None, None),
    "tuner": ([(lr.FrequencyTranslatorBlock, [-250e3]), (lr.LowpassFilterBlock, [128, 100e3]), (lr.DownsamplerBlock, [5])], types.ComplexFloat32, FS,
              "tuner5", None, None),
    "decimator": ([(lr.LowpassFilterBlock, [128, 100e3]), (lr.DownsamplerBlock, [5])], types.ComplexFloat32, FS, "tuner5", None, None),
    "tuner-discriminator": ([(lr.FrequencyTranslatorBlock, [-250e3]), (lr.LowpassFilterBlock, [128, 100e3]), (lr.DownsamplerBlock, [5]),
                             (lr.FrequencyDiscriminatorBlock, [1.25])], types.ComplexFloat32, FS, "tuner5", "disc", None),
    "filter-discriminator": ([(lr.LowpassFilterBlock, [128, 100e3]), (lr.FrequencyDiscriminatorBlock, [1.25])], types.ComplexFloat32, FS, "mfma2d1", None, None),
    "tuner50-magnitude": ([(lr.FrequencyTranslatorBlock, [-350e3]), (lr.LowpassFilterBlock, [128, 10e3]), (lr.DownsamplerBlock, [50]),
                           (lr.ComplexMagnitudeBlock, [])], types.ComplexFloat32, FS, "tuner50", None, None),
    "tuner50-discriminator": ([(lr.FrequencyTranslatorBlock, [-350e3]), (lr.LowpassFilterBlock, [128, 10e3]), (lr.DownsamplerBlock, [50]),
                               (lr.FrequencyDiscriminatorBlock, [1.25])], types.ComplexFloat32, FS, "tuner50", None, None),
    "audio-tail": ([(lr.LowpassFilterBlock, [128, 15e3], {"use_fft": 3}), (lr.FMDeemphasisFilterBlock, [75e-6]), (lr.DownsamplerBlock, [5])], types.Float32,
                   FS / 5, "tail", 1e-6, None),
    "discriminator-fir": ([(lr.FrequencyDiscriminatorBlock, [1.25]), (lr.FIRFilterBlock, [_taps_lp(128, 15e3 / 110250), "fast"])], types.ComplexFloat32, FS / 5,
                          "pass1024r", 1e-6, 1e-6),
    "iir-downsampler-f32": ([(lr.FMDeemphasisFilterBlock, [75e-6]), (lr.DownsamplerBlock, [5])], types.Float32, FS / 5, "iir", None, None),
    "iir-downsampler-cf32": ([(lr.FMDeemphasisFilterBlock, [75e-6]), (lr.DownsamplerBlock, [5])], types.ComplexFloat32, FS / 5, "iir", None, None),
    "phasecorrector-real": ([(lr.BinaryPhaseCorrectorBlock, [50, 32]), (lr.ComplexToRealBlock, [])], types.ComplexFloat32, 1000.0, "pc", None, None),
    "fm-receiver": ([(lr.FrequencyTranslatorBlock, [-250e3]), (lr.LowpassFilterBlock, [128, 100e3]), (lr.DownsamplerBlock, [5]),
                     (lr.FrequencyDiscriminatorBlock, [1.25]), (lr.LowpassFilterBlock, [128, 15e3], {"use_fft": 3}), (lr.FMDeemphasisFilterBlock, [75e-6]),
                     (lr.DownsamplerBlock, [5])], types.ComplexFloat32, FS, "rx", "rms", "rms"),
}


def _fm_signal(n):
    t = np.arange(n) / FS
    msg = 0.5 * np.sin(2 * np.pi * 1e3 * t) + 0.5 * np.sin(2 * np.pi * 5e3 * t)
    return np.exp(1j * (2 * np.pi * 250e3 * t + 2 * np.pi * 75e3 / FS * np.cumsum(msg))).astype(np.complex64)


# In a default chain the LDS-staged decimator splits a rotating Tuner's taps over the half-waves, so the Tuner(.., 50) agrees with its separate blocks to Float32
# rounding only (test_lds_staged_decimator_second_form_many_tiles); the parity tests of what is folded behind it (test_complex_to_real_block_runs_in_the_decimators_store,
# test_lds_staged_decimator_discriminator_epilogue) compare with the same Tuner chain followed by the stand-alone block, bit for bit.  So does the default-mode
# reference of these chains: the first `split` blocks as a chain, the rest one by one.
DEFAULT_REF_SPLIT = {"tuner50-magnitude": 3, "tuner50-discriminator": 3}


def _unfused(specs, in_type, rate, split=0):
    ref = _mk(specs, in_type, rate)
    if split:
        ref = [lr.Chain(ref[:split])] + ref[split:]

    def proc(v):
        for b in ref:
            v = b.process(v)
        return v
    return proc


def _chain_bar(kind, specs, in_type, rate, x):
    """the default-mode bars that are not one tolerance"""
    if kind == "disc":
        # test_discriminator_epilogue_equals_unfused_blocks: disc_err < 2e-6 with the filter outputs as weights, median < 2e-7
        def bar_for(pair):
            filt = chunks(_unfused(specs[:-1], in_type, rate), [x], pair)

            def bar(got, want, c):
                o = filt[c]
                if not len(want):
                    return
                turn = 2 * np.pi / (2 * np.pi * 1.25)
                d = got.astype(np.float64) - want.astype(np.float64)
                d = (d + turn / 2) % turn - turn / 2
                mag = np.abs(o).astype(np.float64)
                w = np.minimum(mag, np.concatenate([mag[:1], mag[:-1]])) / np.sqrt(np.mean(mag ** 2))
                assert float(np.max(np.abs(d) * np.minimum(w, 1.0))) < 2e-6, c
                if len(want) >= 64:
                    assert np.median(np.abs(got - want)) < 2e-7, c
            return bar
        return bar_for
    if kind == "rms":
        # test_wbfm_mono_chain_rms_within_1e5 / smoke(): rms <= 1e-5 against the oracle chain
        def bar_for(pair):
            def bar(got, want, c):
                if len(want):
                    assert float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2))) <= 1e-5, c
            return bar
        return bar_for
    return lambda pair: kind


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chain(name, exact):
    specs, in_type, rate, form, bar, exact_bar = CHAINS[name]
    pairs = len_pairs(T(form))
    n = total(pairs)
    cplx = in_type is types.ComplexFloat32
    x = _fm_signal(n) if name == "fm-receiver" else rand(np.random.default_rng(len(name)), n, cplx)
    out_dtype = _mk(specs, in_type, rate)[-1].get_output_type().dtype
    kind = exact_bar if exact else bar
    bar_for = _chain_bar(kind, specs, in_type, rate, x)
    for pair in pairs:
        if kind == "rms":
            want = chunks(O.wbfm_mono_chain(FS, -250e3, mode=O.MODE_LUA, rot_mode=O.MODE_F64).process, [x], pair)
        else:
            want = chunks(_unfused(specs, in_type, rate, 0 if exact else DEFAULT_REF_SPLIT.get(name, 0)), [x], pair)
        guarded(lambda: lr.Chain(_mk(specs, in_type, rate), exact=exact), [x], lambda p: want, bar_for(pair), [pair], out_dtype=out_dtype)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("tail", [1, 2])
def test_chain_clocksampler_slicer(tail, exact):
    """clocksampler -> slicer [-> differential decoder] (digital_fuse_tail): the count is below the capacity; bit for bit against the model"""
    P = 12500 / 1200
    pairs = len_pairs(T("dg"))
    x = symbols(total(pairs), P, 49)

    def chain():
        specs = [(lr.ClockSamplerBlock, [RATE / P]), (lr.SlicerBlock, [])] + ([(lr.DifferentialDecoderBlock, [True])] if tail == 2 else [])
        return lr.Chain(_mk(specs, types.Float32, RATE), exact=exact)
    counted(chain, [x], lambda: dm.ClockSamplerModel(P, 0.0, *([0.0] if tail == 1 else [0.0, True])).process, pairs, np.uint8)


def _record_source(fmt):
    src = lr.IQFileSource(bytes(16), fmt, FS)
    src.initialize()
    return src


@pytest.mark.parametrize("fmt", ["u8", "s8", "s16le"])
@pytest.mark.parametrize("what", ["tuner", "fm-receiver"])
def test_chain_reads_records_in_place(what, fmt):
    """the Tuner and the single-launch receiver on IQFileSource's u8 / s8 / s16le records (fold_tuner_records, merge_receivers): the hostile input guards
    are 0xFF bytes, the offsets one record.  As in test_tuner_reads_raw_records_in_its_launch and test_receiver_reads_u8_records_in_the_single_launch the
    output has the bits of the same chain fed the converted ComplexFloat32 samples from a device pointer the same number of samples past a 16-byte
    boundary (the receiver's window-relative rotator staging rounds with the alignment slack of its window)"""
    import torch
    specs, in_type, rate, form, _, _ = CHAINS[what]
    pairs = len_pairs(T(form))
    n = total(pairs)
    raw = bytes(O.format_pack(fmt, _fm_signal(n) * np.float32(0.9)))
    rec = np.frombuffer(raw, np.dtype((np.void, 2 * O.FORMAT_BYTES[fmt])))
    xc = O.format_convert(fmt, np.frombuffer(raw, np.uint8), True)
    out_dtype = _mk(specs, in_type, rate)[-1].get_output_type().dtype
    xd = torch.zeros(2 * (n + 8), dtype=torch.float32, device="cuda")
    for io in (0, 1):
        def want(pair):
            ref, out, pos = lr.Chain(_mk(specs, in_type, rate)), [], 0
            for m in pair:                                            # as in the guarded run, every call starts at the same address
                xd[2 * io:2 * (io + m)] = torch.from_numpy(xc[pos:pos + m].view(np.float32).copy()).cuda()
                y = torch.zeros(ref.max_output(m) + 4, dtype=torch.float32 if out_dtype == np.float32 else torch.complex64, device="cuda")
                torch.cuda.synchronize()
                count = ref.process_device(xd.data_ptr() + 8 * io, m, y.data_ptr(), ref.max_output(m))
                _lib.load().lrhip_synchronize()
                out.append(y[:count].cpu().numpy())
                pos += m
            return out
        guarded(lambda: lr.Chain([_record_source(fmt)] + _mk(specs, in_type, rate)), [rec], want, None, pairs, in_offs=(io,), in_kind="raw", out_dtype=out_dtype)


# ===================================================================================================== the three channelizers
@pytest.mark.parametrize("which", ["gemm", "pfb", "oversampled"])
def test_channelizer_reads_only_its_input(which):
    """the channelizers' output guards exist (test_no_write_past_the_count in their own files): here the input side, (d) and (e), with the run's other
    checks along the way"""
    K, M = 32, 96
    L = _lib.load()
    taps = _taps_lp(M, 1.0 / K)
    fp = taps.ctypes.data_as(C.POINTER(C.c_float))
    make_stage = {"gemm": lambda: L.lrhip_channelizer_create(fp, M, K), "pfb": lambda: L.lrhip_pfb_channelizer_create(fp, M, K),
                  "oversampled": lambda: L.lrhip_pfb_oversampled_create(fp, M, K, 2)}[which]
    pairs = [(70 * K + 3, 9 * K + 6), (3, 64 * K + 1)]
    x = rand_c(np.random.default_rng(K + M), total(pairs))
    guarded(lambda: RawStage(make_stage(), which), [x], None, None, pairs, out_dtype=np.complex64)
