"""PreambleSamplerBlock and ManchesterDecoderBlock without a GPU: the models (tests/helpers/ert_model.py) against the reference's golden vectors,
the vectorised preamble sampler against the literal loop, the create-time refusals, and the ERT test signal decoded by a float64 CPU chain."""
import numpy as np
import pytest

from luaradio_amd import blocks as B
from luaradio_amd import composites as comp
from oracle import oracle as O
from tests import golden_util
from tests.helpers import ert_model as em
from tests.helpers import ert_signals as es

RATE = 2.0


def samplewise(model, x):
    parts = [model.process(x[i:i + 1]) for i in range(len(x))]
    return np.concatenate(parts)


def same(a, b):
    """equal as Float32 vectors, NaN equal to NaN, -0.0 apart from 0.0"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32)),
                                                 np.where(np.isnan(b), np.uint32(0x7fc00000), b.view(np.uint32)))


@pytest.mark.parametrize("cls", [em.PreambleSamplerLiteral, em.PreambleSamplerFast])
def test_golden_preamblesampler_models(cls):
    vectors = golden_util.load("preamblesampler_spec")["vectors"]
    assert len(vectors) == 1
    for v in vectors:
        baud, pre, N = v["args"]
        x, want = v["inputs"][0], v["outputs"][0]
        T = int(np.floor(RATE / baud))
        assert (T, len(pre), em.buffer_length(T, len(pre)), len(want)) == (5, 16, 128, 48)
        assert np.array_equal(cls(T, pre, N).process(x), want)
        assert np.array_equal(samplewise(cls(T, pre, N), x), want)


@pytest.mark.parametrize("cls", [em.ManchesterLiteral, em.ManchesterFast])
def test_golden_manchesterdecoder_models(cls):
    vectors = golden_util.load("manchesterdecoder_spec")["vectors"]
    assert len(vectors) == 4
    for v in vectors:
        x, want = np.asarray(v["inputs"][0], np.uint8), np.asarray(v["outputs"][0], np.uint8)
        assert len(want) == 256
        assert np.array_equal(cls(*v["args"]).process(x), want)
        assert np.array_equal(samplewise(cls(*v["args"]), x), want)


def test_preamblesampler_fast_equals_literal_random():
    """300 cases: period 2..6, preamble length 1..5, frame length 2..11, inputs with exact zeros, ties and NaN; outputs and the count of every
    ragged call"""
    rng = np.random.default_rng(2024)
    frames = 0
    for case in range(300):
        T, L, N = int(rng.integers(2, 7)), int(rng.integers(1, 6)), int(rng.integers(2, 12))
        pre = rng.integers(0, 2, L)
        n = int(rng.integers(1, 400))
        x = es.alphabet_signal(n, 1000 + case)
        if case % 3 == 0:                                # mostly matching input: long OPTIMIZING runs and back-to-back frames
            x = np.where(rng.random(n) < 0.8, np.tile(np.repeat(np.where(pre > 0, 1.0, -1.0), T), n // (T * L) + 1)[:n], x).astype(np.float32)
        edges = [0] + sorted(int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 8)))) + [n]
        lit, fast = em.PreambleSamplerLiteral(T, pre, N), em.PreambleSamplerFast(T, pre, N)
        for a, b in zip(edges[:-1], edges[1:]):
            want, got = lit.process(x[a:b]), fast.process(x[a:b])
            assert same(got, want), (case, T, L, N, a, b)
        frames += len(fast.frames)
    assert frames > 1000


def test_manchester_fast_equals_literal_random():
    rng = np.random.default_rng(5)
    for case in range(200):
        n = int(rng.integers(0, 300))
        x = rng.integers(0, 256, n).astype(np.uint8) if case % 2 else np.repeat(rng.integers(0, 2, n // 2 + 1), 2)[:n].astype(np.uint8)
        edges = [0] + sorted(int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 6)))) + [n]
        lit, fast = em.ManchesterLiteral(case % 3 == 0), em.ManchesterFast(case % 3 == 0)
        for a, b in zip(edges[:-1], edges[1:]):
            assert np.array_equal(fast.process(x[a:b]), lit.process(x[a:b])), (case, a, b)


def test_preamblesampler_constructor_refusals():
    pre = [0, 1, 1]
    assert B.preamble_sampler_params(10.0, 2.0, pre, 8) == (5, 3, 8, 16)
    assert B.preamble_sampler_params(2.0, 0.4, np.array(pre, np.uint8), 48)[0] == 5
    with pytest.raises(ValueError, match="period"):
        B.preamble_sampler_params(10.0, 8.0, pre, 8)                 # T = 1
    with pytest.raises(ValueError, match="num_samples"):
        B.preamble_sampler_params(10.0, 2.0, pre, 1)
    with pytest.raises(ValueError, match="empty"):
        B.preamble_sampler_params(10.0, 2.0, [], 8)
    with pytest.raises(TypeError):
        B.preamble_sampler_params(10.0, 2.0, [0, 2, 1], 8)
    with pytest.raises(TypeError):
        B.preamble_sampler_params(10.0, 2.0, "0101", 8)
    with pytest.raises(ValueError, match="limit"):
        B.preamble_sampler_params(float(1 << 21), 1.0, [1], 8)       # T L = 2^21: B = 2^22
    assert B.preamble_sampler_params(float(1 << 20), 1.0, [1], 8)[3] == 1 << 21      # T L = 2^20 is admitted
    with pytest.raises(AssertionError, match="#1"):
        B.PreambleSamplerBlock(None, pre, 8)
    with pytest.raises(AssertionError, match="#2"):
        B.PreambleSamplerBlock(2.0, None, 8)
    with pytest.raises(AssertionError, match="#3"):
        B.PreambleSamplerBlock(2.0, pre, None)
    blk = B.PreambleSamplerBlock(2.0, pre, 8)
    blk.rate = 10.0
    assert blk.op() == "preamblesampler:period=5:num_samples=8:preamble=011"
    assert B.ManchesterDecoderBlock(True).op() == "manchesterdecoder:invert=1"
    for model in (em.PreambleSamplerLiteral, em.PreambleSamplerFast):
        for bad in ((1, pre, 8), (5, pre, 1), (5, [], 8)):
            with pytest.raises(ValueError):
                model(*bad)


def test_ert_receiver_constants_and_protocol_check():
    assert (len(comp.IDM_PREAMBLE), len(comp.SCM_PREAMBLE), len(comp.SCM_PLUS_PREAMBLE)) == (32, 21, 16)
    assert comp.IDM_PREAMBLE[16:] == comp.SCM_PLUS_PREAMBLE
    assert (comp.IDM_FRAME_LEN, comp.SCM_FRAME_LEN, comp.SCM_PLUS_FRAME_LEN) == (736, 96, 128)
    with pytest.raises(ValueError, match="Unsupported protocol"):
        comp.ert_receiver(("scm", "r900"), rate=es.ERT_RATE)


def cpu_front_end(x):
    """ComplexMagnitude -> Lowpass(128, 131072) -> Downsampler(6) -> ManchesterMatchedFilter(32768), float64 accumulation"""
    mag = np.abs(x.astype(np.complex128)).astype(np.float32)
    y = O.lowpass(128, 4 * 32768, es.ERT_RATE, False, mode=O.MODE_F64).process(mag)
    y = O.Downsampler(es.ERT_DECIMATION, False).process(y)
    half = int(es.ERT_RATE / es.ERT_DECIMATION / 32768)
    return O.FIR(np.array([-1.0] * half + [1.0] * half, np.float32), False, mode=O.MODE_F64).process(y)


@pytest.mark.parametrize("sigma", [0.0, 0.02, 0.05, 0.1])
def test_ert_signal_is_decodable_on_the_cpu(sigma):
    x, frames = es.ert_signal(sigma)
    assert 200000 < len(x) < 230000
    mf = cpu_front_end(x)
    want = es.ert_expected(frames)
    assert len(want["scm"]) == 2 * 96 and len(want["scm+"]) == 2 * 128 and len(want["idm"]) == 736
    T = 24
    smallest = np.inf
    for proto, (pre, N) in comp.ERT_PROTOCOLS.items():
        s = em.PreambleSamplerFast(T, pre, N).process(mf)
        assert np.array_equal((s > 0).astype(np.uint8), want[proto]), proto
        smallest = min(smallest, float(np.min(np.abs(s))))
    # far from the slicer's threshold: Float32 rounding in a device front end cannot flip a bit
    assert smallest > 9.0 if sigma <= 0.05 else smallest > 5.0, smallest
