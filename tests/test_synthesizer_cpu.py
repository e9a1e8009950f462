"""CPU side of the polyphase + FFT synthesis filterbank (PolyphaseSynthesizerBlock, "pfbsynthesizer:..." of lrhip_unary_create): the float64
reference of tests/helpers/synthesizer_ref.py against the defining sum, against the analysis bank's conventions (an exact identity) and in the
near-perfect-reconstruction pair it forms with the oversampled analysis bank; the op string and the shapes the constructor refuses (before the
device is touched); and the Lua block under the Lua interpreter of tests/helpers/minilua.py."""
import numpy as np
import pytest

from luaradio_amd import _lib, filter_utils
from tests.helpers import channelizer_os_ref as OS
from tests.helpers import lua_mocks as LM
from tests.helpers import minilua as ml
from tests.helpers import synthesizer_ref as SR

SHAPES = [(8, 23, 1), (8, 23, 2), (8, 27, 4), (16, 50, 4), (8, 8, 1)]


def _frames(rng, F, K, scale=1.0):
    return (scale * (rng.standard_normal((F, K)) + 1j * rng.standard_normal((F, K)))).astype(np.complex64)


def _stream(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.parametrize("K,M,R", SHAPES)
def test_polyphase_equals_literal_sum(K, M, R):
    """the polyphase form against the K chains term by term, to 1e-12 relative (of B[n], the sum of the absolute terms)"""
    rng = np.random.default_rng(100 * K + M + R)
    Y = _frames(rng, 3 * ((M + K // R - 1) // (K // R)) + 5, K, 1e3)
    g = rng.uniform(-1, 1, M).astype(np.float32)
    x, B = SR.synthesize_f64(Y, g, K, R)
    lit = SR.synthesize_literal(Y, g, K, R)
    assert x.shape == lit.shape == (len(Y) * K // R,) and np.all(B > 0)
    assert np.all(np.abs(x - lit) <= 1e-12 * B)


@pytest.mark.parametrize("K,M,R", SHAPES)
def test_f32_emulation_is_near_the_reference(K, M, R):
    """the Float32 restatement that sets the device tests' aggregate bar: inside the per-output bar, and an rms ratio of order one"""
    rng = np.random.default_rng(7 * K + M + R)
    Y = _frames(rng, 64, K)
    g = rng.uniform(-1, 1, M).astype(np.float32)
    x, B = SR.synthesize_f64(Y, g, K, R)
    emu = SR.synthesize_f32_emulation(Y, g, K, R)
    assert emu.dtype == np.complex64
    D = K // R
    r = SR.check_bars(emu, x, B, K, (M + D - 1) // D, 4.0)
    assert r > 0.01


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("K", [8, 16])
def test_exact_identity_with_the_analysis_bank(K, R):
    """h = [0, 1, ..., 1] (K + 1 taps) on the analysis side and g = ones(K) / K: xhat[n] = R x[n - K] exactly, which pins the channel order, the
    sign of the transform, the rotation and the delay against the analysis bank's conventions"""
    rng = np.random.default_rng(K + R)
    D = K // R
    n = 37 * K + 3
    x = _stream(rng, n)
    h = np.concatenate([[0.0], np.ones(K)]).astype(np.float32)
    Y, _ = OS.channelize_os_f64(x, h, K, R)
    xhat, _ = SR.synthesize_f64(Y, np.full(K, 1.0 / K, np.float32), K, R)
    assert len(xhat) == len(Y) * D >= n
    want = np.concatenate([np.zeros(K), R * x.astype(np.complex128)])[:len(xhat)]
    assert float(np.max(np.abs(xhat[:n] - want[:n]))) < 1e-13 * R * float(np.max(np.abs(x)))


def rrc_round_trip(K, R, beta, n):
    """(best-fit scale, residual of xhat K / R against x delayed by M - 1, relative) of analysis -> synthesis with one RRC prototype, in float64"""
    M = 16 * K + 1
    h = np.asarray(filter_utils.fir_root_raised_cosine(M, 1.0, beta, K), np.float32)
    x = _stream(np.random.default_rng(1000 * K + R), n)
    Y, _ = OS.channelize_os_f64(x, h, K, R)
    xhat, _ = SR.synthesize_f64(Y, h, K, R)
    got, want = xhat[M - 1:n], x.astype(np.complex128)[:n - (M - 1)]
    scale = (np.vdot(want, got) / np.vdot(want, want)).real
    resid = float(np.linalg.norm(got * K / R - want) / np.linalg.norm(want))
    return float(scale), resid


@pytest.mark.parametrize("K,R,beta", [(16, 2, 0.5), (16, 4, 1.0), (8, 2, 0.5), (64, 2, 0.5)])
def test_rrc_round_trip_reconstructs(K, R, beta):
    """a root-raised-cosine prototype of 16 K + 1 taps on both sides of an oversampled pair returns (R / K) x[n - (M - 1)]: the scale within 1e-3,
    the residual at most 2e-3; the same pair critically sampled aliases (residual above 0.1), which is what oversampling buys"""
    n = 96 * K
    scale, resid = rrc_round_trip(K, R, beta, n)
    print("rrc round trip K=%d R=%d beta=%g: scale K / R = %.6f residual %.3e" % (K, R, beta, scale * K / R, resid))
    assert abs(scale * K / R - 1) <= 1e-3
    assert resid <= 2e-3
    _, crit = rrc_round_trip(K, 1, beta, n)
    assert crit > 0.1


def _python_block(K, taps, options=None):
    import luaradio_amd as lr
    from luaradio_amd import types
    blk = lr.PolyphaseSynthesizerBlock(K, taps, options)
    blk.rate = 48000.0
    blk.differentiate([types.ComplexFloat32])
    return blk


def parse_op(op):
    head, channels, oversample, taps = op.split(":")
    assert head == "pfbsynthesizer" and channels.startswith("channels=") and oversample.startswith("oversample=") and taps.startswith("taps=")
    return int(channels[9:]), int(oversample[11:]), np.array([float(t) for t in taps[5:].split(",")]).astype(np.float32)


def test_op_string_keeps_the_taps_exactly():
    rng = np.random.default_rng(11)
    taps = (rng.standard_normal(23) * 1e-3).astype(np.float32)
    taps[3], taps[4] = np.float32(1e-30), np.float32(-3.4e38)
    for R in (1, 2, 4):
        blk = _python_block(8, taps, {"oversample": R})
        K, r, got = parse_op(blk.op())
        assert (K, r) == (8, R) and np.array_equal(got, taps)
        assert blk.get_rate() == 48000.0 / R
    blk = _python_block(16, None)
    assert blk.oversample == 1 and len(blk.taps) == 256
    assert np.array_equal(parse_op(blk.op())[2], np.asarray(filter_utils.firwin_lowpass(256, 1.0 / 16), np.float32))


def test_python_block_assertions():
    import luaradio_amd as lr
    with pytest.raises(AssertionError, match="num_channels"):
        lr.PolyphaseSynthesizerBlock(None)
    for bad in (0, 3, 8, "2"):
        with pytest.raises(AssertionError, match="oversample"):
            lr.PolyphaseSynthesizerBlock(64, np.ones(64, np.float32), {"oversample": bad})


def _create(op):
    L = _lib.load()
    return L, L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 1)


def _op(K, R, ntaps):
    return "pfbsynthesizer:channels=%d:oversample=%d:taps=%s" % (K, R, ",".join(["0.5"] * ntaps))


@pytest.mark.parametrize("op,rule", [
    (_op(64, 0, 1024), "oversample must be 1, 2 or 4"), (_op(64, 3, 1024), "oversample must be 1, 2 or 4"), (_op(64, 8, 1024), "oversample must be 1, 2 or 4"),
    (_op(0, 2, 64), "nchannels must be a power of two in [8, 4096]"), (_op(4, 2, 64), "nchannels must be a power of two in [8, 4096]"),
    (_op(48, 4, 96), "nchannels must be a power of two in [8, 4096]"), (_op(8192, 2, 8192), "nchannels must be a power of two in [8, 4096]"),
    (_op(64, 4, 63), "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"), (_op(8, 4, 7), "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"),
    (_op(8, 2, 64 * 8 + 1), "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"), (_op(4096, 2, 65537), "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"),
    (_op(4096, 1, 4095), "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"),
    ("pfbsynthesizer:channels=8:oversample=2:taps=", "ntaps must be in"),
    ("pfbsynthesizer:channels=8:oversample=2:taps=1,2,x,4,5,6,7,8", "bad tap 2"),
    ("pfbsynthesizer:channels=8:oversample=2:taps=1,2,3,4,5,6,7,8,", "end with a comma"),
    ("pfbsynthesizer:channels=8:oversample=2:taps=1,2,3,4,5,6,7,8 9", "bad tap 7"),
    ("pfbsynthesizer:channels=8:oversample=2:taps=1,2,,4,5,6,7,8", "bad tap 2"),
    ("pfbsynthesizer:channels=8x:oversample=2:taps=1,2,3,4,5,6,7,8", "bad value for \"channels\""),
    ("pfbsynthesizer:channels=8:oversample=2", "missing parameter \"taps\""),
    ("pfbsynthesizer:channels=8:taps=1,2,3,4,5,6,7,8", "missing parameter \"oversample\""),
    ("pfbsynthesizer:channels=8:oversample=2:taps=1,2,3,4,5,6,7,8:extra=1", "unknown parameter \"extra\""),
    ("pfbsynthesizer:channels=8:channels=8:oversample=2:taps=1,2,3,4,5,6,7,8", "given twice"),
    ("pfbsynthesizer", "missing parameter \"channels\""),
])
def test_create_refusals(op, rule):
    """the analysis bank's domain, and an op string that is not well formed: refused with the rule, before the device is touched (this test
    runs without one)"""
    L, st = _create(op)
    assert not st
    msg = L.lrhip_strerror().decode()
    assert msg.startswith("pfb_synthesizer: ") and rule in msg, msg


LUA_BLOCK = r'''
local types = require('radio.types')
local k, taps, oversample = ...
local C = require('radio.blocks.signal.channelizer_hip').PolyphaseSynthesizerBlock
local b = C(k, taps, {oversample = oversample})
b:differentiate({types.ComplexFloat32})
b:initialize()
return b
'''


def _lua_block(K, taps, oversample):
    I, proxy, _ = LM.make_interpreter()
    vec = LM.Vector(LM.DataType("Float32", np.float32), 0, np.asarray(taps, np.float32).copy())
    b = I.run(LUA_BLOCK, "pfb_synth", [float(K), vec, None if oversample is None else float(oversample)])[0]
    x = LM.Vector(LM.DataType("ComplexFloat32", np.complex64), 0, np.zeros(10 * K, np.complex64))
    ml.call(ml.index(b, "process"), [b, x])
    ml.call(ml.index(b, "process"), [b, x])
    return b, [a for n, a in proxy.fake.calls if n == "lrhip_unary_create"]


def test_lua_block_creates_the_stage_by_name():
    """one lrhip_unary_create call however many vectors are processed; its op string parses back to the Float32 taps; get_rate() is rate / R"""
    rng = np.random.default_rng(12)
    taps = (rng.standard_normal(50) * 1e-3).astype(np.float32)
    rate = r'''
    local b, r = ...
    b.inputs[1].pipe = {get_rate = function () return r end}
    return b:get_rate()
    '''
    for R in (None, 1, 2, 4):
        b, creates = _lua_block(16, taps, R)
        assert len(creates) == 1
        op = creates[0][0]
        op = op.decode() if isinstance(op, bytes) else str(op)
        K, r, got = parse_op(op)
        assert (K, r) == (16, R or 1) and np.array_equal(got, taps)
        assert [int(v) for v in creates[0][1:]] == [0, 0, 0, 1]
        I, _, _ = LM.make_interpreter()
        assert I.run(rate, "rate", [b, 48000.0])[0] == 48000.0 / (R or 1)
    for bad in (0, 3, 8):
        with pytest.raises(Exception, match="Unsupported oversample"):
            _lua_block(16, taps, bad)
