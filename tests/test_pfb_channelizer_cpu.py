"""CPU side of the polyphase + FFT channelizer: the shapes lrhip_pfb_channelizer_create refuses (before the device is touched), the float64
reference of tests/helpers/channelizer_ref.py on the ground the new form opens (K = 8 and 256, M not a multiple of K) against the defining
sum, and the Lua block's choice of entry point under the Lua interpreter of tests/helpers/minilua.py."""
import ctypes as C

import numpy as np
import pytest

from luaradio_amd import _lib
from tests.helpers import channelizer_ref as CR
from tests.helpers import lua_mocks as LM
from tests.helpers import minilua as ml

K_RULE = "nchannels must be a power of two in [8, 4096]"
M_RULE = "ntaps must be in [nchannels, min(64 * nchannels, 65536)]"


@pytest.mark.parametrize("ntaps,nch,rule", [
    (64, 0, K_RULE), (64, 4, K_RULE), (96, 48, K_RULE), (96, 96, K_RULE), (8192, 8192, K_RULE),
    (0, 64, M_RULE), (63, 64, M_RULE), (7, 8, M_RULE), (64 * 64 + 1, 64, M_RULE), (64 * 8 + 1, 8, M_RULE), (65537, 4096, M_RULE), (4095, 4096, M_RULE),
])
def test_pfb_channelizer_refusals(ntaps, nch, rule):
    """the accepted domain is K a power of two in [8, 4096] and K <= M <= min(64 K, 65536); anything else is refused with its rule"""
    L = _lib.load()
    taps = np.ones(max(ntaps, 1), np.float32)
    assert not L.lrhip_pfb_channelizer_create(taps.ctypes.data_as(C.POINTER(C.c_float)), ntaps, nch)
    msg = L.lrhip_strerror().decode()
    assert msg.startswith("pfb_channelizer: ") and rule in msg, msg


def test_pfb_channelizer_refuses_null_taps():
    L = _lib.load()
    assert not L.lrhip_pfb_channelizer_create(C.POINTER(C.c_float)(), 1024, 64)
    assert M_RULE in L.lrhip_strerror().decode()


@pytest.mark.parametrize("K,M", [(8, 8), (8, 9), (8, 23), (8, 509), (256, 257), (256, 767), (256, 300)])
def test_reference_equals_literal_sum_on_the_new_ground(K, M):
    """the yardstick of tests/test_gpu_pfb_channelizer.py where those tests use it: the polyphase fold with the prototype padded to whole
    rows against the definition term by term, to 1e-12 of B[m]; small blocks so that the block loop is crossed"""
    rng = np.random.default_rng(11 * K + M)
    n = 5 * K + 3
    x = (1e3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    h = rng.uniform(-1, 1, M).astype(np.float32)
    y, B = CR.channelize_f64(x, h, K, block_elems=2 * M)
    lit = CR.channelize_literal(x, h, K)
    assert y.shape == (CR.nframes(n, K), K) and np.all(B > 0)
    assert np.all(np.abs(y - lit) <= 1e-12 * B[:, None])


LUA_BLOCK = r'''
local types = require('radio.types')
local k, taps, method = ...
local C = require('radio.blocks.signal.channelizer_hip').PolyphaseChannelizerBlock
local b
if method == nil then b = C(k, taps) else b = C(k, taps, {method = method}) end
b:differentiate({types.ComplexFloat32})
b:initialize()
return b
'''


PFB = "lrhip_pfb_channelizer_create"


def _lua_creates(K, ntaps, method, without_fft=False):
    """the stage constructors called by building the Lua block and processing one vector.  Loading the block's file probes the library for
    the FFT form with one call that creates nothing (no taps, no channels), before anything touches the device; it is checked and left out."""
    I, proxy, _ = LM.make_interpreter()
    if without_fft:
        proxy.sigs = {k: v for k, v in proxy.sigs.items() if k != PFB}          # an older liblrhip.so
    taps = LM.Vector(LM.DataType("Float32", np.float32), 0, np.ones(ntaps, np.float32))
    b = I.run(LUA_BLOCK, "pfb", [float(K), taps, method])[0]
    x = LM.Vector(LM.DataType("ComplexFloat32", np.complex64), 0, np.zeros(10 * K, np.complex64))
    y = ml.call(ml.index(b, "process"), [b, x])[0]
    assert y.length == 10 * K
    calls = [(n, a) for n, a in proxy.fake.calls if n.endswith("channelizer_create")]
    if without_fft:
        assert PFB not in proxy.trace
    else:
        assert calls[0] == (PFB, [None, 0, 0]) and proxy.trace.count("lrhip_init") == 1 and proxy.trace.index(PFB) < proxy.trace.index("lrhip_init")
        calls = calls[1:]
    return [(n, a[1:]) for n, a in calls]


def test_lua_block_picks_the_entry_point_by_method():
    """{method = "fft"} -> lrhip_pfb_channelizer_create(#taps, K), also where the GEMM would accept the shape; no options or "gemm" on a
    GEMM shape -> lrhip_channelizer_create; a shape the GEMM refuses (K = 256; K = 64 with 1000 taps) without options -> the FFT form;
    "gemm" outside its domain still asks the GEMM, whose refusal the caller then sees"""
    assert _lua_creates(64, 1024, "fft") == [("lrhip_pfb_channelizer_create", [1024, 64])]
    assert _lua_creates(64, 1024, None) == [("lrhip_channelizer_create", [1024, 64])]
    assert _lua_creates(64, 1024, "gemm") == [("lrhip_channelizer_create", [1024, 64])]
    assert _lua_creates(256, 4096, None) == [("lrhip_pfb_channelizer_create", [4096, 256])]
    assert _lua_creates(64, 1000, None) == [("lrhip_pfb_channelizer_create", [1000, 64])]
    assert _lua_creates(256, 4096, "gemm") == [("lrhip_channelizer_create", [4096, 256])]
    with pytest.raises(Exception, match="Unsupported method"):
        _lua_creates(64, 1024, "dft")


def test_lua_block_on_a_library_without_the_fft_form():
    """the glue may meet an older liblrhip.so: the block is then the GEMM alone, as it was - "fft" raises, a shape outside the GEMM's domain
    is handed to the GEMM's constructor, whose refusal the caller sees"""
    assert _lua_creates(64, 1024, None, without_fft=True) == [("lrhip_channelizer_create", [1024, 64])]
    assert _lua_creates(256, 4096, None, without_fft=True) == [("lrhip_channelizer_create", [4096, 256])]
    with pytest.raises(Exception, match="no lrhip_pfb_channelizer_create"):
        _lua_creates(64, 1024, "fft", without_fft=True)


def test_python_block_picks_the_entry_point_by_method(monkeypatch):
    """the same rule in luaradio_amd.PolyphaseChannelizerBlock, seen at the library boundary (no device: the constructors are replaced)"""
    import luaradio_amd as lr
    from luaradio_amd import types

    class Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if not name.endswith("channelizer_create"):
                raise AttributeError(name)
            return lambda taps, ntaps, nch: self.calls.append((name, ntaps, nch)) or 0x1000

    def created(K, ntaps, options):
        lib = Lib()
        monkeypatch.setattr(_lib, "load", lambda: lib)
        blk = lr.PolyphaseChannelizerBlock(K, np.ones(ntaps, np.float32), options) if options is not None else lr.PolyphaseChannelizerBlock(K, np.ones(ntaps, np.float32))
        monkeypatch.setattr(blk, "_set_stage", lambda handle, what: None)
        blk.differentiate([types.ComplexFloat32])
        blk.initialize()
        return lib.calls

    assert created(64, 1024, None) == [("lrhip_channelizer_create", 1024, 64)]
    assert created(32, 96, {}) == [("lrhip_channelizer_create", 96, 32)]
    assert created(64, 1024, {"method": "gemm"}) == [("lrhip_channelizer_create", 1024, 64)]
    assert created(64, 1024, {"method": "fft"}) == [("lrhip_pfb_channelizer_create", 1024, 64)]
    assert created(256, 4096, None) == [("lrhip_pfb_channelizer_create", 4096, 256)]
    assert created(64, 1000, None) == [("lrhip_pfb_channelizer_create", 1000, 64)]
    assert created(64, 16384, None) == [("lrhip_pfb_channelizer_create", 16384, 64)]
    assert created(256, 4096, {"method": "gemm"}) == [("lrhip_channelizer_create", 4096, 256)]
    with pytest.raises(AssertionError, match="Unsupported method"):
        lr.PolyphaseChannelizerBlock(64, np.ones(64, np.float32), {"method": "dft"})
