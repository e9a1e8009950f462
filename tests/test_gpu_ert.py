"""PreambleSamplerBlock, ManchesterDecoderBlock and ert_receiver on the MI355X, bit for bit against the Python models
(tests/helpers/ert_model.py): the reference's golden vectors, random inputs in ragged chunks (every chunk's output, not only the
concatenation), long stretches without a match and without a degradation, state, refusals, chains, and the receiver end to end."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from luaradio_amd import composites as comp
from tests import golden_util
from tests.helpers import ert_model as em
from tests.helpers import ert_signals as es

pytestmark = pytest.mark.gpu

RATE = 2.0


def make(cls, args, in_types, rate=RATE):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate(in_types)
    blk.initialize()
    return blk


def sampler(T, pre, N):
    """PreambleSamplerBlock with symbol period T: baudrate 1 at rate T"""
    return make(lr.PreambleSamplerBlock, [1.0, pre, N], [types.Float32], rate=float(T))


def bits_of(a):
    """Float32 vectors by their bits (the data has NaNs and -0.0); every NaN the same"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def assert_chunks_equal(blk, model, x, edges, bound=None):
    for a, b in zip(edges[:-1], edges[1:]):
        got, want = blk.process(x[a:b]), model.process(x[a:b])
        if bound is not None:
            assert len(got) <= bound(b - a)
        if want.dtype == np.float32:
            assert got.dtype == np.float32 and np.array_equal(bits_of(got), bits_of(want)), (a, b, len(got), len(want))
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want), (a, b, len(got), len(want))


# ---- golden vectors ------------------------------------------------------------------------------------------------------------------
def test_golden_preamblesampler():
    for v in golden_util.load("preamblesampler_spec")["vectors"]:
        x, want = v["inputs"][0], v["outputs"][0]
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: make(lr.PreambleSamplerBlock, v["args"], [types.Float32]), x)
        assert len(want) == 48
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)


def test_golden_manchesterdecoder():
    for v in golden_util.load("manchesterdecoder_spec")["vectors"]:
        x, want = np.asarray(v["inputs"][0], np.uint8), np.asarray(v["outputs"][0], np.uint8)
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: make(lr.ManchesterDecoderBlock, v["args"], [types.Bit]), x)
        assert len(want) == 256 and whole.dtype == np.uint8
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)


# ---- PreambleSampler, random ---------------------------------------------------------------------------------------------------------
def random_case(T, L, N, n, seed):
    rng = np.random.default_rng(seed)
    pre = rng.integers(0, 2, L).astype(np.uint8)
    if not pre.any():
        pre[-1] = 1
    x = es.alphabet_signal(n, seed + 1)
    if L >= 16:                                          # a random match of 16 and more taps is rare: plant frames, some cut short, some back to back
        at = 3 * T * L
        while at < n - T:
            amp = float(rng.choice([1.0, 0.5, 0.25]))
            at = es.plant_frame(x, at, T, pre, int(rng.choice([N, N, L + 2, 2 * N])), rng, amp) + int(rng.choice([0, 1, T, 7 * T * N]))
    return pre, x


@pytest.mark.parametrize("T,L,N,n", [(2, 1, 2, 1 << 18), (3, 3, 5, 1 << 16), (5, 16, 48, 1 << 16), (24, 21, 96, 1 << 20)])
def test_preamblesampler_random(T, L, N, n):
    pre, x = random_case(T, L, N, n, 100 * T + L)
    scout = em.PreambleSamplerFast(T, pre, N)
    whole = scout.process(x)
    assert len(scout.frames) >= 8 and len(whole) >= 8 * N - N, len(scout.frames)
    if T == 2:
        assert len(whole) > n // 8                       # dense frames: the T = 2 bound matters
    edges = es.ragged_cuts(n, scout.frames, scout.B, T, N, seed=T)
    assert any(b - a == 1 for a, b in zip(edges[:-1], edges[1:])) and any(b == a for a, b in zip(edges[:-1], edges[1:]))
    blk = sampler(T, pre, N)
    assert blk.max_output(1001) == (1001 if T == 2 else 502)
    assert_chunks_equal(blk, em.PreambleSamplerFast(T, pre, N), x, edges, bound=blk.max_output)
    # the same block again from its initial state, in one call
    blk.reset()
    assert np.array_equal(bits_of(blk.process(x)), bits_of(whole))


def test_preamblesampler_random_small_vs_literal_loop():
    """the literal loop itself as the reference, at sizes it can run: odd lengths, one-sample calls"""
    T, L, N, n = 3, 2, 4, 3001
    pre, x = random_case(T, L, N, n, 77)
    rng = np.random.default_rng(1)
    edges = [0] + sorted(int(c) for c in rng.integers(0, n, 40)) + [n - 3, n - 2, n - 1, n]
    assert_chunks_equal(sampler(T, pre, N), em.PreambleSamplerLiteral(T, pre, N), x, edges)


def test_preamblesampler_three_tiles_and_an_event_on_the_last_sample():
    """n = 2 * 1024 + 1: three tiles of the match pass, an odd count, where the two 4-byte lists of tile summaries need padding in front of
    the frame list of the scratch; the third tile holds the last sample alone, and the last frame's j* falls on it"""
    T, N, n = 3, 20, 2 * 1024 + 1
    pre = np.array([0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1], np.uint8)
    rng = np.random.default_rng(333)
    x = es.alphabet_signal(n, 334)
    es.plant_frame(x, 100, T, pre, N, rng)               # a frame in the first tile
    es.plant_frame(x, n - 65, T, pre, N, rng)            # B = 64: the window lags behind the input, this frame's j* is sample n - 1
    scout = em.PreambleSamplerFast(T, pre, N)
    scout.process(x)
    assert len(scout.frames) == 2 and scout.frames[0][1] < 1024 and scout.frames[1][1] == n - 1
    blk = sampler(T, pre, N)
    assert_chunks_equal(blk, em.PreambleSamplerLiteral(T, pre, N), x, [0, n])
    blk.reset()
    assert_chunks_equal(blk, em.PreambleSamplerLiteral(T, pre, N), x, [0, n - 30, n])


def test_preamblesampler_long_quiet_stretches():
    T, N = 3, 5
    pre = np.array([0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1], np.uint8)
    n = 1 << 22
    x = np.full(n, -1.0, np.float32)
    blk = sampler(T, pre, N)
    assert len(blk.process(x)) == 0                      # never matches: the walk crosses 4096 tiles by their summaries
    # then one frame at the very end of the next call
    rng = np.random.default_rng(3)
    end = es.plant_frame(x, n - T * (len(pre) + 6), T, pre, len(pre) + 4, rng)
    assert end <= n
    model = em.PreambleSamplerFast(T, pre, N)
    assert len(model.process(np.full(n, -1.0, np.float32))) == 0
    want = model.process(x)
    assert 1 <= len(want) < N and len(model.frames) == 1          # found in the call's last samples; the frame ends in the next call
    assert np.array_equal(bits_of(blk.process(x)), bits_of(want))
    rest = model.process(x[:64])
    assert len(want) + len(rest) == N
    assert np.array_equal(bits_of(blk.process(x[:64])), bits_of(rest))
    # M holds and E never degrades: OPTIMIZING runs through the whole call and the next, and ends at the first smaller sample
    blk, model = sampler(2, [1], 2), em.PreambleSamplerFast(2, [1], 2)
    ones = np.ones(1 << 16, np.float32)
    tail = np.array([1.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)      # B = 4: the window lags two samples behind the input
    for part in (ones, ones, tail):
        got, want = blk.process(part), model.process(part)
        assert np.array_equal(bits_of(got), bits_of(want))
    assert model.frames[0] == (2, 2 * len(ones) + 3) and len(want) == 2


def test_preamblesampler_state_reset_and_independent_blocks():
    T, L, N, n = 5, 16, 48, 1 << 14
    pre, x = random_case(T, L, N, n, 9)
    want = em.PreambleSamplerFast(T, pre, N).process(x)
    assert len(want) > N
    a, b = sampler(T, pre, N), sampler(T, pre, N)
    cut = em.PreambleSamplerFast(T, pre, N)
    cut.process(x)
    mid = cut.frames[1][1] + 2 * T                       # inside a frame
    first = a.process(x[:mid])
    assert np.array_equal(bits_of(b.process(x)), bits_of(want))       # b is not disturbed by a's half-finished frame
    assert np.array_equal(bits_of(np.concatenate([first, a.process(x[mid:])])), bits_of(want))
    a.process(x[:mid])
    a.reset()
    assert np.array_equal(bits_of(a.process(x)), bits_of(want))


@pytest.mark.parametrize("op,what", [
    ("preamblesampler:period=1:num_samples=8:preamble=01", "period"),
    ("preamblesampler:period=5:num_samples=1:preamble=01", "num_samples"),
    ("preamblesampler:period=5:num_samples=8:preamble=", "empty"),
    ("preamblesampler:period=5:num_samples=8:preamble=0121", "0 / 1"),
    ("preamblesampler:period=5:num_samples=8:preamble=01:threshold=0", "unknown parameter"),
    ("preamblesampler:period=5:num_samples=8", "missing parameter"),
    ("preamblesampler:period=5.5:num_samples=8:preamble=01", "integer"),
    ("preamblesampler:period=2097152:num_samples=8:preamble=1", "limit"),
    ("manchesterdecoder:invert=2", "invert"),
    ("manchesterdecoder:invert=0:period=2", "unknown parameter"),
    ("manchesterdecoder", "missing parameter"),
])
def test_refusals(op, what):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    assert what in L.lrhip_strerror().decode(), L.lrhip_strerror().decode()


def test_refusals_through_the_blocks():
    with pytest.raises(ValueError, match="period"):
        make(lr.PreambleSamplerBlock, [2.0, [0, 1], 8], [types.Float32], rate=2.0)
    with pytest.raises(TypeError):
        lr.PreambleSamplerBlock(1.0, [0, 3], 8)
    ok = _lib.load().lrhip_unary_create(b"preamblesampler:period=1048576:num_samples=2:preamble=1", 0.0, 0.0, 0, 0)      # T L = 2^20 is admitted
    assert ok
    _lib.load().lrhip_stage_destroy(ok)


# ---- ManchesterDecoder, random -------------------------------------------------------------------------------------------------------
def manchester_input(n, seed, slips):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, n // 2 + 1).astype(np.uint8)
    x = np.stack([data, 1 - data], axis=1).reshape(-1)
    pos = np.sort(rng.choice(len(x), size=slips, replace=False))
    x = np.insert(x, pos, x[pos])[:n]                    # a repeated bit: a clock slip
    return (x | (rng.integers(0, 128, n).astype(np.uint8) << 1)).astype(np.uint8)       # only bit 0 of a byte counts


@pytest.mark.parametrize("n", [1 << 16, 1 << 22])
@pytest.mark.parametrize("invert", [False, True])
def test_manchesterdecoder_random(n, invert):
    x = manchester_input(n, n + invert, n // 200)
    rng = np.random.default_rng(4)
    cuts = set(int(c) for c in rng.integers(1, n, 6)) | {1, 2, 4097, 4098, n // 2, n // 2 + 1, n - 1}      # odd and even: some split a pair
    edges = [0] + sorted(cuts) + [n]
    blk = make(lr.ManchesterDecoderBlock, [invert], [types.Bit])
    assert blk.max_output(1001) == 501
    assert_chunks_equal(blk, em.ManchesterFast(invert), x, edges, bound=blk.max_output)


@pytest.mark.parametrize("invert", [False, True])
def test_manchesterdecoder_odd_length_vs_literal_loop(invert):
    """n = 2 * 1024 + 1 against the literal loop, whole and cut once inside the last pair, into the same block after reset()"""
    n = 2 * 1024 + 1
    x = manchester_input(n, 333 + invert, 10)
    blk = make(lr.ManchesterDecoderBlock, [invert], [types.Bit])
    assert len(em.ManchesterLiteral(invert).process(x)) >= 2
    assert_chunks_equal(blk, em.ManchesterLiteral(invert), x, [0, n])
    blk.reset()
    assert_chunks_equal(blk, em.ManchesterLiteral(invert), x, [0, n - 2, n])


def test_manchesterdecoder_degenerate_inputs_and_one_sample_calls():
    n = 10001
    for invert in (False, True):
        blk = make(lr.ManchesterDecoderBlock, [invert], [types.Bit])
        assert len(blk.process(np.ones(n, np.uint8))) == 0 and len(blk.process(np.ones(n, np.uint8))) == 0        # all equal: nothing
        blk.reset()
        alt = (np.arange(n - 1) & 1).astype(np.uint8)
        got = blk.process(alt)
        assert len(got) == (n - 1) // 2 and np.array_equal(got, np.full((n - 1) // 2, 1 if invert else 0, np.uint8))
        x = manchester_input(600, 5, 20)
        blk.reset()
        lit = em.ManchesterLiteral(invert)
        assert_chunks_equal(blk, lit, x, list(range(len(x) + 1)))
        blk.reset()
        assert np.array_equal(blk.process(x), em.ManchesterLiteral(invert).process(x))


# ---- in a chain and a graph ----------------------------------------------------------------------------------------------------------
def chain_cases():
    T, L, N, n = 5, 16, 48, 1 << 17
    pre, x = random_case(T, L, N, n, 21)
    return T, pre, N, x


def test_chain_preamblesampler_slicer_and_slicer_manchester():
    T, pre, N, x = chain_cases()
    n = len(x)
    edges = [0, 1, 5000, 5001, 77777, n]
    ps, sl = sampler(T, pre, N), make(lr.SlicerBlock, [], [types.Float32])
    want = np.concatenate([sl.process(ps.process(x[a:b])) for a, b in zip(edges[:-1], edges[1:])])
    assert np.array_equal(want, (em.PreambleSamplerFast(T, pre, N).process(x) > 0).astype(np.uint8)) and len(want) > 10 * N
    ch = comp.Chain([sampler(T, pre, N), make(lr.SlicerBlock, [], [types.Float32])])
    assert ch.max_output(1001) == 502
    got = np.concatenate([ch.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    with pytest.raises(lr.LrhipError):
        ch.start_at(4096)
    # Slicer -> ManchesterDecoder on a noisy Manchester wave
    bits = manchester_input(n, 8, 300) & 1
    wave = ((bits.astype(np.float32) * 2 - 1) * 0.7 + 0.1 * np.random.default_rng(2).standard_normal(n)).astype(np.float32)
    sl, md = make(lr.SlicerBlock, [], [types.Float32]), make(lr.ManchesterDecoderBlock, [True], [types.Bit])
    want = np.concatenate([md.process(sl.process(wave[a:b])) for a, b in zip(edges[:-1], edges[1:])])
    assert np.array_equal(want, em.ManchesterFast(True).process((wave > 0).astype(np.uint8))) and len(want) > n // 3
    ch = comp.Chain([make(lr.SlicerBlock, [], [types.Float32]), make(lr.ManchesterDecoderBlock, [True], [types.Bit])])
    got = np.concatenate([ch.process(wave[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert np.array_equal(got, want)
    with pytest.raises(lr.LrhipError):
        ch.start_at(4096)


def test_chain_ring_and_push():
    T, pre, N, x = chain_cases()
    n, chunk, depth = len(x), 20000, 4
    want = (em.PreambleSamplerFast(T, pre, N).process(x) > 0).astype(np.uint8)
    ch = comp.Chain([sampler(T, pre, N), make(lr.SlicerBlock, [], [types.Float32])])
    ch.set_ring(depth, chunk)
    got = np.concatenate(list(ch.stream(x[a:a + chunk] for a in range(0, n, chunk))))
    assert np.array_equal(got, want)
    ch = comp.Chain([sampler(T, pre, N), make(lr.SlicerBlock, [], [types.Float32])])
    ch.set_ring(depth, chunk)
    parts = [ch.push(x[a:a + 7001]) for a in range(0, n, 7001)]
    parts.append(ch.flush())
    assert np.array_equal(np.concatenate(parts), want)
    # Slicer -> ManchesterDecoder under the ring
    bits = manchester_input(n, 8, 300) & 1
    wave = (bits.astype(np.float32) - 0.5).astype(np.float32)
    ch = comp.Chain([make(lr.SlicerBlock, [], [types.Float32]), make(lr.ManchesterDecoderBlock, [False], [types.Bit])])
    ch.set_ring(depth, chunk)
    got = np.concatenate(list(ch.stream(wave[a:a + chunk] for a in range(0, n, chunk))))
    assert np.array_equal(got, em.ManchesterFast(False).process(bits))


def test_preamblesampler_in_device_graph():
    T, pre, N, x = chain_cases()
    x = x[:1 << 15]
    g = lr.DeviceGraph()
    src = g.input("in", types.Float32, float(T))
    g.connect(src, lr.PreambleSamplerBlock(1.0, pre, N), lr.SlicerBlock())
    g.initialize()
    edges = [0, 3, 4, 9999, len(x)]
    got = np.concatenate([g.process(**{"in": x[a:b]})["SlicerBlock"] for a, b in zip(edges[:-1], edges[1:])])
    assert np.array_equal(got, (em.PreambleSamplerFast(T, pre, N).process(x) > 0).astype(np.uint8))


# ---- ert_receiver end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ert_case():
    x, frames = es.ert_signal(0.05)
    return x, es.ert_expected(frames)


def test_ert_receiver_end_to_end(ert_case):
    x, want = ert_case
    assert 200000 < len(x) < 230000
    rx = lr.ert_receiver(rate=es.ERT_RATE, decimation=es.ERT_DECIMATION)
    got = rx.process(**{"in": x})
    assert sorted(got) == ["idm", "scm", "scm+"]
    assert len(want["scm"]) == 192 and len(want["idm"]) == 736 and len(want["scm+"]) == 256
    for proto in want:
        assert got[proto].dtype == np.uint8 and np.array_equal(got[proto], want[proto]), proto


def test_ert_receiver_ragged_chunks_and_protocol_subset(ert_case):
    x, want = ert_case
    rng = np.random.default_rng(6)
    edges = [0] + sorted(int(c) for c in rng.integers(1, len(x), 9)) + [len(x)]
    rx = lr.ert_receiver(rate=es.ERT_RATE)
    parts = [rx.process(**{"in": x[a:b]}) for a, b in zip(edges[:-1], edges[1:])]
    for proto in want:
        assert np.array_equal(np.concatenate([p[proto] for p in parts]), want[proto]), proto
    one = lr.ert_receiver(("scm",), rate=es.ERT_RATE)
    got = one.process(**{"in": x})
    assert list(got) == ["scm"] and np.array_equal(got["scm"], want["scm"])
    with pytest.raises(ValueError, match="Unsupported protocol"):
        lr.ert_receiver(("scm", "r900"), rate=es.ERT_RATE)
    # existing graphs keep their keys
    assert list(lr.pocsag_receiver().process(**{"in": np.zeros(80 * 64, np.complex64)})) == ["SlicerBlock"]
