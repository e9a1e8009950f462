"""CPU side of the channelizer: the float64 filterbank of tests/helpers/channelizer_ref.py against the pinned oracle chains
Rotator(-2 pi c / K) -> FIR(h) -> Downsampler(K) and against the defining sum term by term, and the shapes lrhip_channelizer_create refuses."""
import numpy as np
import pytest

from luaradio_amd import _lib
from oracle import oracle as O
from tests.helpers import channelizer_ref as CR

U = CR.U32

SHAPES = [(4, 3), (4, 4), (8, 20), (8, 32), (16, 16), (32, 96), (32, 40), (64, 32), (64, 96)]


def _stream(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _taps(rng, M, K, kind):
    if kind == "lowpass":
        return O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    return rng.uniform(-1, 1, M).astype(np.float32)


@pytest.mark.parametrize("kind", ["lowpass", "random"])
@pytest.mark.parametrize("K,M", SHAPES)
def test_reference_equals_oracle_chains(K, M, kind):
    """Each oracle chain rounds the rotated samples and its own output to Float32 (the phasor too), so it sits within
    2^-24 (2 B[m] + |y|) of the exact filterbank per component; the float64 reference must land inside that, over a ragged stream"""
    rng = np.random.default_rng(1000 * K + M)
    n = 23 * K + 5                                   # not a multiple of K: the last frame reads a partial hop
    x = _stream(rng, n)
    h = _taps(rng, M, K, kind)
    y, B = CR.channelize_f64(x, h, K)
    assert y.shape == (CR.nframes(n, K), K) and B.shape == (y.shape[0],)
    for c in range(K):
        want = O.Chain([O.Rotator(-2 * np.pi * c / K, O.MODE_F64), O.FIR(h, True, O.MODE_F64), O.Downsampler(K, True)]).process(x)
        assert want.shape == (y.shape[0],)
        w = want.astype(np.complex128)
        for part in (np.real, np.imag):
            lim = U * (2 * B + np.abs(part(y[:, c]))) * (1 + 1e-9) + 1e-12 * B
            err = np.abs(part(w) - part(y[:, c]))
            assert np.all(err <= lim), (c, int(np.argmax(err / lim)), float(np.max(err / lim)))


@pytest.mark.parametrize("K,M", SHAPES + [(32, 33), (64, 200)])
def test_reference_equals_literal_sum(K, M):
    """the FFT of the polyphase fold against the definition term by term, to 1e-12 of B[m]; small blocks so the block loop is crossed"""
    rng = np.random.default_rng(7 * K + M)
    n = 9 * K + 3
    x = _stream(rng, n, 1e3)
    h = _taps(rng, M, K, "random")
    y, B = CR.channelize_f64(x, h, K, block_elems=2 * M)
    lit = CR.channelize_literal(x, h, K)
    assert np.all(np.abs(y - lit) <= 1e-12 * B[:, None])


def test_reference_b_and_conventions():
    """frame m ends at sample mK (downsampler phase 0), samples before the stream are zero, B is the l1 weight of the window"""
    K, M = 4, 6
    h = np.array([1, -2, 3, -4, 5, -6], np.float32)
    x = np.zeros(10, np.complex64)
    x[5] = 1 - 2j
    y, B = CR.channelize_f64(x, h, K)
    assert y.shape == (3, K)
    # frames 0 and 1 end before sample 5; frame 2 holds it at i = 8 - 5 = 3
    assert np.all(y[0] == 0) and np.all(y[1] == 0)
    c = np.arange(K)
    assert np.allclose(y[2], -4 * (1 - 2j) * np.exp(2j * np.pi * c * 3 / K), rtol=0, atol=1e-12)
    assert np.array_equal(B, [0.0, 0.0, 4 * 3.0])
    y0, B0 = CR.channelize_f64(np.zeros(0, np.complex64), h, K)
    assert y0.shape == (0, K) and B0.shape == (0,)


@pytest.mark.parametrize("ntaps,nch,rule", [
    (0, 64, "ntaps"), (31, 64, "ntaps"), (33, 64, "ntaps"), (8224, 64, "ntaps"), (8192 + 1, 32, "ntaps"),
    (64, 16, "nchannels"), (64, 48, "nchannels"), (64, 128, "nchannels"), (64, 0, "nchannels"),
])
def test_channelizer_refusals(ntaps, nch, rule):
    """the accepted domain is K in {32, 64}, M a multiple of 32 in [32, 8192]; anything else is refused before the device is touched"""
    import ctypes as C
    L = _lib.load()
    taps = np.ones(max(ntaps, 1), np.float32)
    assert not L.lrhip_channelizer_create(taps.ctypes.data_as(C.POINTER(C.c_float)), ntaps, nch)
    msg = L.lrhip_strerror().decode()
    if rule == "ntaps":
        assert "ntaps must be a multiple of 32 in [32, 8192]" in msg, msg
    else:
        assert "nchannels must be 32 or 64" in msg, msg
