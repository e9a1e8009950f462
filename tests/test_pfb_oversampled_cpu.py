"""CPU side of the oversampled polyphase + FFT channelizer (lrhip_pfb_oversampled_create, hop D = K / R): the float64 reference of
tests/helpers/channelizer_os_ref.py against the oracle's K chains and against the defining sum, its agreement with the critically sampled
reference where the two coincide, the shapes the constructor refuses (before the device is touched), and the choice of entry point in the
Python block and in the Lua block under the Lua interpreter of tests/helpers/minilua.py."""
import ctypes as C

import numpy as np
import pytest

from luaradio_amd import _lib
from oracle import oracle as O
from tests.helpers import channelizer_os_ref as OS
from tests.helpers import channelizer_ref as CR
from tests.helpers import lua_mocks as LM
from tests.helpers import minilua as ml

U = CR.U32
SHAPES = [(4, 3, 2), (8, 20, 2), (8, 32, 4), (16, 16, 4), (32, 40, 2), (64, 96, 4)]
OS_RULE = "oversample must be 1, 2 or 4"
K_RULE = "nchannels must be a power of two in [8, 4096]"
M_RULE = "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"
NEW = "lrhip_pfb_oversampled_create"


def _stream(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _taps(rng, M, K, kind):
    if kind == "lowpass":
        return O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    return rng.uniform(-1, 1, M).astype(np.float32)


@pytest.mark.parametrize("kind", ["lowpass", "random"])
@pytest.mark.parametrize("K,M,R", SHAPES)
def test_reference_equals_oracle_chains(K, M, R, kind):
    """Each oracle chain Rotator(-2 pi c / K) -> FIR(h) -> Downsampler(D) rounds the rotated samples and its own output to Float32 (the phasor
    too), so it sits within 2^-24 (2 B[m] + |y|) of the exact filterbank per component; the float64 reference must land inside that, for every
    channel, over a stream that ends inside a hop"""
    rng = np.random.default_rng(1000 * K + 10 * M + R)
    D = K // R
    n = 23 * D + 5
    x = _stream(rng, n)
    h = _taps(rng, M, K, kind)
    y, B = OS.channelize_os_f64(x, h, K, R)
    assert y.shape == (OS.nframes(n, D), K) and B.shape == (y.shape[0],)
    for c in range(K):
        want = O.Chain([O.Rotator(-2 * np.pi * c / K, O.MODE_F64), O.FIR(h, True, O.MODE_F64), O.Downsampler(D, True)]).process(x)
        assert want.shape == (y.shape[0],)
        w = want.astype(np.complex128)
        for part in (np.real, np.imag):
            lim = U * (2 * B + np.abs(part(y[:, c]))) * (1 + 1e-9) + 1e-12 * B
            err = np.abs(part(w) - part(y[:, c]))
            assert np.all(err <= lim), (c, int(np.argmax(err / lim)), float(np.max(err / lim)))


@pytest.mark.parametrize("K,M,R", SHAPES + [(8, 23, 2), (8, 8, 4), (16, 50, 4), (64, 200, 2)])
def test_reference_equals_literal_sum(K, M, R):
    """the rotated polyphase fold against the definition term by term, to 1e-12 of B[m]; small blocks so that the block loop is crossed"""
    rng = np.random.default_rng(7 * K + M + R)
    n = 9 * K + 3
    x = _stream(rng, n, 1e3)
    h = _taps(rng, M, K, "random")
    y, B = OS.channelize_os_f64(x, h, K, R, block_elems=2 * M)
    lit = OS.channelize_os_literal(x, h, K, R)
    assert y.shape == lit.shape and np.all(B > 0)
    assert np.all(np.abs(y - lit) <= 1e-12 * B[:, None])


@pytest.mark.parametrize("K,M", [(8, 23), (16, 16), (64, 1000)])
def test_rate_one_is_the_critically_sampled_reference(K, M):
    rng = np.random.default_rng(K + M)
    x = _stream(rng, 31 * K + 7)
    h = _taps(rng, M, K, "random")
    y, B = OS.channelize_os_f64(x, h, K, 1)
    y1, B1 = CR.channelize_f64(x, h, K)
    assert np.array_equal(y, y1) and np.array_equal(B, B1)


@pytest.mark.parametrize("K,M,R", [(8, 23, 2), (8, 8, 4), (16, 50, 4), (64, 1000, 2)])
def test_frames_m_r_are_the_critically_sampled_frames(K, M, R):
    """frame m R has the window of the critically sampled frame m and rotation 0: the same y exactly, the same B to the last bits"""
    rng = np.random.default_rng(3 * K + M + R)
    x = _stream(rng, 31 * K + 7)
    h = _taps(rng, M, K, "random")
    y, B = OS.channelize_os_f64(x, h, K, R)
    y1, B1 = CR.channelize_f64(x, h, K)
    assert len(y[::R]) == len(y1)
    assert np.array_equal(y[::R], y1)
    assert np.allclose(B[::R], B1, rtol=1e-14, atol=0)           # a matrix-vector product: the summation order may depend on the row count


def _create(taps, ntaps, nch, R):
    L = _lib.load()
    p = taps.ctypes.data_as(C.POINTER(C.c_float)) if taps is not None else C.POINTER(C.c_float)()
    return L, L.lrhip_pfb_oversampled_create(p, ntaps, nch, R)


@pytest.mark.parametrize("ntaps,nch,R,rule", [
    (1024, 64, 0, OS_RULE), (1024, 64, 3, OS_RULE), (1024, 64, 8, OS_RULE), (0, 0, 0, OS_RULE),
    (64, 0, 2, K_RULE), (64, 4, 2, K_RULE), (96, 48, 4, K_RULE), (8192, 8192, 2, K_RULE),
    (0, 64, 2, M_RULE), (63, 64, 4, M_RULE), (7, 8, 4, M_RULE), (64 * 8 + 1, 8, 2, M_RULE), (65537, 4096, 2, M_RULE), (4095, 4096, 1, M_RULE),
])
def test_oversampled_refusals(ntaps, nch, R, rule):
    """the domain of the FFT form plus oversample in {1, 2, 4}; anything else is refused with its rule, before the device is touched (this
    test runs without one)"""
    L, st = _create(np.ones(max(ntaps, 1), np.float32), ntaps, nch, R)
    assert not st
    msg = L.lrhip_strerror().decode()
    assert msg.startswith("pfb_channelizer: ") and rule in msg, msg


def test_oversampled_refuses_null_taps():
    L, st = _create(None, 1024, 64, 2)
    assert not st
    assert M_RULE in L.lrhip_strerror().decode()


class _Lib:
    """a library boundary that records the channelizer constructors"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in ("lrhip_channelizer_create", "lrhip_pfb_channelizer_create", NEW):
            raise AttributeError(name)
        return lambda taps, *args: self.calls.append((name,) + args) or 0x1000


def _python_block(monkeypatch, K, ntaps, options):
    import luaradio_amd as lr
    from luaradio_amd import types
    lib = _Lib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    blk = lr.PolyphaseChannelizerBlock(K, np.ones(ntaps, np.float32), options)
    monkeypatch.setattr(blk, "_set_stage", lambda handle, what: None)
    blk.rate = 48000.0
    blk.differentiate([types.ComplexFloat32])
    blk.initialize()
    return blk, lib.calls


def test_python_block_routes_oversample(monkeypatch):
    """oversample 2 or 4 with no method or "fft" -> lrhip_pfb_oversampled_create(#taps, K, R), also on a shape the GEMM accepts; "gemm" raises;
    oversample 1 is the block as it was; any other value is an assertion error that names the option"""
    import luaradio_amd as lr
    assert _python_block(monkeypatch, 64, 1024, {"oversample": 2})[1] == [(NEW, 1024, 64, 2)]
    assert _python_block(monkeypatch, 64, 1024, {"method": "fft", "oversample": 2})[1] == [(NEW, 1024, 64, 2)]
    assert _python_block(monkeypatch, 8, 23, {"oversample": 4})[1] == [(NEW, 23, 8, 4)]
    with pytest.raises(ValueError, match="critically sampled only"):
        _python_block(monkeypatch, 64, 1024, {"method": "gemm", "oversample": 2})
    assert _python_block(monkeypatch, 64, 1024, {"oversample": 1})[1] == [("lrhip_channelizer_create", 1024, 64)]
    assert _python_block(monkeypatch, 64, 1024, {"method": "fft", "oversample": 1})[1] == [("lrhip_pfb_channelizer_create", 1024, 64)]
    for bad in (0, 3, 8, "2"):
        with pytest.raises(AssertionError, match="oversample"):
            lr.PolyphaseChannelizerBlock(64, np.ones(64, np.float32), {"oversample": bad})


def test_python_block_rate(monkeypatch):
    """the port carries R * rate values per second"""
    for R in (1, 2, 4):
        blk, _ = _python_block(monkeypatch, 64, 1024, {"oversample": R})
        assert blk.get_rate() == 48000.0 * R
    assert _python_block(monkeypatch, 64, 1024, None)[0].get_rate() == 48000.0


LUA_BLOCK = r'''
local types = require('radio.types')
local k, taps, method, oversample = ...
local C = require('radio.blocks.signal.channelizer_hip').PolyphaseChannelizerBlock
local b = C(k, taps, {method = method, oversample = oversample})
b:differentiate({types.ComplexFloat32})
b:initialize()
return b
'''


def _lua_creates(K, ntaps, method, oversample, without=()):
    """the stage constructors called by building the Lua block and processing one vector, the load-time probes (which create nothing and come
    before lrhip_init) left out"""
    I, proxy, _ = LM.make_interpreter()
    proxy.sigs = {k: v for k, v in proxy.sigs.items() if k not in without}          # an older liblrhip.so
    taps = LM.Vector(LM.DataType("Float32", np.float32), 0, np.ones(ntaps, np.float32))
    b = I.run(LUA_BLOCK, "pfb_os", [float(K), taps, method, None if oversample is None else float(oversample)])[0]
    x = LM.Vector(LM.DataType("ComplexFloat32", np.complex64), 0, np.zeros(10 * K, np.complex64))
    ml.call(ml.index(b, "process"), [b, x])
    calls = [(n, a[1:]) for n, a in proxy.fake.calls if n == NEW or n.endswith("channelizer_create")]
    probes = [c for c in calls if c[1] in ([0, 0], [0, 0, 0])]
    if NEW not in without:
        assert (NEW, [0, 0, 0]) in probes and proxy.trace.index(NEW) < proxy.trace.index("lrhip_init")
    else:
        assert NEW not in proxy.trace
    return [c for c in calls if c not in probes], b


def test_lua_block_routes_oversample():
    """options.oversample = 2 -> lrhip_pfb_oversampled_create(#taps, K, 2) for no method and "fft", also on a GEMM shape; "gemm" raises;
    oversample 1 or absent leaves the choice as it was; get_rate is multiplied by R"""
    assert _lua_creates(64, 1024, None, 2)[0] == [(NEW, [1024, 64, 2])]
    assert _lua_creates(64, 1024, "fft", 2)[0] == [(NEW, [1024, 64, 2])]
    assert _lua_creates(8, 23, None, 4)[0] == [(NEW, [23, 8, 4])]
    assert _lua_creates(64, 1024, None, 1)[0] == [("lrhip_channelizer_create", [1024, 64])]
    assert _lua_creates(64, 1024, "fft", None)[0] == [("lrhip_pfb_channelizer_create", [1024, 64])]
    assert _lua_creates(256, 4096, None, 1)[0] == [("lrhip_pfb_channelizer_create", [4096, 256])]
    with pytest.raises(Exception, match="critically sampled only"):
        _lua_creates(64, 1024, "gemm", 2)
    for bad in (0, 3, 8):
        with pytest.raises(Exception, match="Unsupported oversample"):
            _lua_creates(64, 1024, None, bad)


def test_lua_block_rate():
    rate = r'''
    local b, r = ...
    b.inputs[1].pipe = {get_rate = function () return r end}
    return b:get_rate()
    '''
    for R in (None, 1, 2, 4):
        b = _lua_creates(64, 1024, "fft", R)[1]
        I, _, _ = LM.make_interpreter()
        assert I.run(rate, "rate", [b, 48000.0])[0] == 48000.0 * (R or 1)


def test_lua_block_on_a_library_without_the_oversampled_form():
    """an older liblrhip.so: oversample 2 gives the clear error, everything else is as it was"""
    with pytest.raises(Exception, match="this liblrhip.so has no lrhip_pfb_oversampled_create"):
        _lua_creates(64, 1024, None, 2, without=(NEW,))
    assert _lua_creates(64, 1024, None, None, without=(NEW,))[0] == [("lrhip_channelizer_create", [1024, 64])]
    assert _lua_creates(64, 1024, "fft", 1, without=(NEW,))[0] == [("lrhip_pfb_channelizer_create", [1024, 64])]
    assert _lua_creates(256, 4096, None, None, without=(NEW,))[0] == [("lrhip_pfb_channelizer_create", [4096, 256])]
    assert _lua_creates(64, 1024, None, None, without=(NEW, "lrhip_pfb_channelizer_create"))[0] == [("lrhip_channelizer_create", [1024, 64])]
