"""ConvolutionalEncoderBlock and ViterbiDecoderBlock on the MI355X, bit for bit against the model (tests/helpers/viterbi_model.py): every lane layout
(S < 64, one, two and four states per lane), hard input, ties and special values, every chunking, reset, seek and time partitions, pointers off 16
bytes, guard words, the capacity check, and the loopback through the modulator and the soft demodulator as Chains, in a DeviceGraph and on the ring.

Unless a case says otherwise the shape is D = 64, L = 24: windows of 112 steps (two chunks of 64 in the kernel, the second one partial), streams of
five windows and 5 steps."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, timeshard, types
from tests.helpers import demodulator_models as dm
from tests.helpers import guarded as GD
from tests.helpers import modulator_model as mm
from tests.helpers import viterbi_model as vm
from tests.test_gpu_bounds import TorchMemory, device_call

pytestmark = pytest.mark.gpu

D, L = 64, 24
# K, polynomials, depth
CODES = {"k3": (3, [0o7, 0o5], L), "k7": (7, [0o171, 0o133], L), "k7-third": (7, [0o133, 0o171, 0o165], L), "k8": (8, [0o247, 0o371], L),
         "k9": (9, [0o561, 0o753], 32)}


def steps(depth, windows=5, extra=5):
    return windows * D + depth + extra


def encoder(K, polys):
    blk = lr.ConvolutionalEncoderBlock(K, polys)
    blk.rate = 1.0
    blk.differentiate([types.Bit])
    blk.initialize()
    return blk


def decoder(K, polys, depth=L, soft=True, scale=8.0, block=D):
    """(block, model)"""
    blk = lr.ViterbiDecoderBlock(K, polys, {"soft": soft, "scale": scale, "block": block, "depth": depth})
    blk.rate = float(len(polys))
    blk.differentiate([types.Float32 if soft else types.Bit])
    blk.initialize()
    return blk, vm.DecoderModel(K, polys, soft, scale, block, depth)


def noisy_llrs(rng, K, polys, nsteps, ebn0_db=1.0):
    msg = rng.integers(0, 2, nsteps).astype(np.uint8)
    return msg, vm.awgn_llrs(rng, vm.encode(K, polys, msg), ebn0_db, 1.0 / len(polys))


_REFERENCE = {}


def k7_reference():
    """one noisy K = 7 stream and the model's bits, shared by the tests that cut, seek and move it"""
    if not _REFERENCE:
        K, polys, _ = CODES["k7"]
        rng = np.random.default_rng(77)
        msg, x = noisy_llrs(rng, K, polys, steps(L, windows=7))
        want = vm.DecoderModel(K, polys, True, 8.0, D, L).process(x)
        want.setflags(write=False)
        x.setflags(write=False)
        _REFERENCE.update(x=x, want=want)
    return _REFERENCE["x"], _REFERENCE["want"]


@pytest.mark.parametrize("name", list(CODES))
def test_encoder_and_decoder_against_the_model(name):
    K, polys, depth = CODES[name]
    rng = np.random.default_rng(K * 10 + len(polys))
    n = len(polys)
    msg = rng.integers(0, 256, steps(depth)).astype(np.uint8)              # bytes with junk above bit 0: the stages read bit 0
    enc = encoder(K, polys)
    code = enc.process(msg)
    assert enc.max_output(len(msg)) == n * len(msg)
    assert code.dtype == np.uint8 and np.array_equal(code, vm.encode(K, polys, msg & 1))
    x = vm.awgn_llrs(rng, code, 1.0, 1.0 / n)
    blk, model = decoder(K, polys, depth)
    got, want = blk.process(x), model.process(x)
    assert got.dtype == np.uint8 and len(want) == 5 * D
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert 0 < np.count_nonzero(np.sign(x) != 1 - 2.0 * code)              # the channel did flip code bits
    assert np.count_nonzero(got != (msg & 1)[:len(got)]) < len(got) // 4


def test_encoder_history_across_calls_and_seek():
    K, polys, _ = CODES["k9"]
    msg = np.random.default_rng(3).integers(0, 2, 700).astype(np.uint8)
    want = vm.encode(K, polys, msg)
    enc = encoder(K, polys)
    parts = [enc.process(msg[a:b]) for a, b in zip([0, 0, 1, 3, 10, 300, 300], [0, 1, 3, 10, 300, 300, 700])]
    assert np.array_equal(np.concatenate(parts), want)
    enc.reset()
    assert np.array_equal(enc.process(msg[:9]), want[:18])
    # a seek forgets the K - 1 bits in front: the output is the stream's again memory() = K - 1 bits later
    enc.seek(100)
    got = enc.process(msg[100:])
    assert np.array_equal(got[2 * (K - 1):], want[2 * (100 + K - 1):]) and np.array_equal(got, vm.encode(K, polys, msg[100:]))
    chain = lr.Chain([enc])
    assert chain.halo() == K - 1
    parts = [timeshard.run_partition(chain, msg, a, b, align=1) for a, b in [(0, 5), (5, 333), (333, 700)]]
    assert np.array_equal(np.concatenate(parts), want)


def test_hard_input():
    K, polys, _ = CODES["k7"]
    rng = np.random.default_rng(8)
    msg = rng.integers(0, 2, steps(L)).astype(np.uint8)
    code = vm.encode(K, polys, msg)
    flips = rng.random(len(code)) < 0.04
    x = (code ^ flips).astype(np.uint8) | (rng.integers(0, 128, len(code)).astype(np.uint8) << 1)      # junk above bit 0
    blk, model = decoder(K, polys, soft=False)
    got, want = blk.process(x), model.process(x & 1)
    assert np.array_equal(got, want) and len(got) == 5 * D
    assert np.array_equal(got, msg[:len(got)])


def special_streams(name, n_values, rng, scale):
    if name == "zeros":
        return np.zeros(n_values, np.float32)
    if name == "ties":
        return (rng.integers(-1, 2, n_values) / scale).astype(np.float32)
    if name == "halves":
        return (rng.choice([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5], n_values) / scale).astype(np.float32)
    x = (3.0 * rng.standard_normal(n_values)).astype(np.float32)
    if name == "non-finite":
        where = rng.choice(n_values, n_values // 5, replace=False)
        x[where] = rng.choice(np.array([np.nan, np.inf, -np.inf, -np.nan], np.float32), len(where))
    else:
        x *= np.float32(1e3)                                                # "saturated": nearly all beyond +-127, some beyond Float32
        x[::7] = np.float32(3e38)
        x[3::11] = np.float32(-3e38)
    return x


@pytest.mark.parametrize("name", ["zeros", "ties", "halves", "non-finite", "saturated"])
@pytest.mark.parametrize("code", ["k7", "k9", "k3"])
def test_ties_and_special_values(code, name):
    K, polys, depth = CODES[code]
    rng = np.random.default_rng(len(name))
    x = special_streams(name, len(polys) * steps(depth), rng, 8.0)
    q = vm.quantise(x, 8.0)
    if name == "halves":
        assert set(np.unique(q)) == {-2, 0, 2}                             # ties to even
    if name == "non-finite":
        assert np.isnan(x).sum() > 20 and np.isinf(x).sum() > 20 and (q[np.isnan(x)] == 0).all() and (np.abs(q[np.isinf(x)]) == 127).all()
    if name == "saturated":
        assert (np.abs(q) == 127).mean() > 0.9
    blk, model = decoder(K, polys, depth)
    got, want = blk.process(x), model.process(x)
    assert len(want) == 5 * D and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    if name == "zeros":
        assert not got.any()                                               # every comparison ties: b = 0, the lowest state


def cut(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


@pytest.mark.parametrize("chunk", ["whole", 1, 7, 2 * D - 1, 2 * (D + L) + 1, "ragged"])
def test_any_chunking_gives_the_same_bytes(chunk):
    K, polys, _ = CODES["k7"]
    x, want = k7_reference()
    if chunk == 1:
        x, want = x[:2 * steps(L)], want[:5 * D]                            # (five windows and 5 steps: two launches per input value)
    sizes = [len(x)] if chunk == "whole" else [0, 5, 0, 0, 2 * (D + L) - 5, 1, 0, 2 * D, len(x) - 4 * D - 2 * L - 1] if chunk == "ragged" else cut(len(x), chunk)
    assert sum(sizes) == len(x)
    blk, _ = decoder(K, polys)
    for _ in range(2):
        parts, pos = [], 0
        for size in sizes:
            got = blk.process(x[pos:pos + size])
            assert len(got) <= blk.max_output(size) and len(got) % D == 0
            parts.append(got)
            pos += size
        got = np.concatenate(parts)
        assert np.array_equal(got, want), (chunk, len(got), len(want))
        assert chunk not in (1, 7, "ragged") or any(len(p) == 0 for p in parts)
        blk.reset()                                                        # and the same again


def test_seek_and_time_partitions():
    K, polys, _ = CODES["k7"]
    n = len(polys)
    x, want = k7_reference()
    blk, model = decoder(K, polys)
    M = n * (D + 2 * L) - 1
    assert blk.memory() == M == vm.memory(n, D, L)
    chain = lr.Chain([blk])
    assert chain.halo() == M and chain.shard_align() == 1
    rng = np.random.default_rng(4)
    fresh = rng.standard_normal(M + n * (2 * D + 3)).astype(np.float32)
    # the block is the model wherever it is started: the carried inputs are erasures
    for n0 in (0, 1, 2, 3, n * (D + L), n * (D + L) + 1, 5 * n * D + 7, (1 << 40) + 3, (1 << 40) + 2 * D * n):
        blk.process(fresh[:9])                                             # another partition's position
        blk.seek(n0)
        model.seek(n0)
        got, expect = blk.process(fresh), model.process(fresh)
        assert len(expect) >= D and np.array_equal(got, expect), n0
    # behind memory() inputs the output is the uninterrupted stream's, at the same absolute positions; one input earlier it need not be
    for n0 in (1, 2, n * (D - L), n * (D - L) + 1, n * D + 5, 3 * n * D - 1):
        blk.seek(n0)
        head = blk.process(x[n0:n0 + M])
        tail = blk.process(x[n0 + M:])
        first = vm.bits_done(n0 + M, n, D, L)
        assert first == vm.bits_done(n0, n, D, L) + len(head)
        assert len(tail) >= D and np.array_equal(tail, want[first:]), n0
    cuts = sorted({0, 1, 2 * (D + L), 2 * (D + L) + 1, 401, 402, 4 * D * n + 3, len(x)})
    parts = [timeshard.run_partition(chain, x, a, b, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), want)
    assert len(parts[0]) == 0 and sum(len(p) > 0 for p in parts) >= 3
    for G in (2, 3):
        parts = [timeshard.run_partition(chain, x, a, b) for a, b in timeshard.bounds(len(x), G, align=1)]
        assert np.array_equal(np.concatenate(parts), want)


@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
def test_pointers_off_16_bytes(soft):
    import torch
    K, polys, _ = CODES["k7"]
    rng = np.random.default_rng(6)
    msg, llr = noisy_llrs(rng, K, polys, steps(L))
    x = llr if soft else (llr < 0).astype(np.uint8)
    blk, model = decoder(K, polys, soft=soft)
    want = model.process(x)
    enc = encoder(K, polys)
    size = x.dtype.itemsize
    for in_off in (0, 1, 3):
        for out_off in (0, 1, 2, 5):
            xt = torch.zeros(len(x) * size + 64, dtype=torch.uint8, device="cuda")
            xt[in_off * size:(in_off + len(x)) * size] = torch.from_numpy(x.view(np.uint8)).cuda()
            yt = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            blk.reset()
            count = blk.process_device(xt.data_ptr() + in_off * size, len(x), yt.data_ptr() + out_off, len(want))
            _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
            raw = yt.cpu().numpy()
            assert count == len(want) and np.array_equal(raw[out_off:out_off + len(want)], want), (in_off, out_off)
            assert not raw[:out_off].any() and not raw[out_off + len(want):].any()
    for in_off, out_off in ((1, 0), (0, 3), (5, 1)):
        mt = torch.zeros(len(msg) + 64, dtype=torch.uint8, device="cuda")
        mt[in_off:in_off + len(msg)] = torch.from_numpy(msg).cuda()
        yt = torch.zeros(2 * len(msg) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.reset()
        count = enc.process_device(mt.data_ptr() + in_off, len(msg), yt.data_ptr() + out_off, 2 * len(msg))
        _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
        raw = yt.cpu().numpy()
        assert count == 2 * len(msg) and np.array_equal(raw[out_off:out_off + count], vm.encode(K, polys, msg))
        assert not raw[:out_off].any() and not raw[out_off + count:].any()


@pytest.mark.parametrize("code,soft", [("k7", True), ("k7", False), ("k9", True), ("k3", True)])
def test_guard_words_decoder(code, soft):
    """tests/helpers/guarded.py, as tests/test_gpu_bounds.py runs it: nothing is written before the output or behind the count, every output of the
    count is written, the input is untouched, and hostile words behind the call's n values change nothing"""
    K, polys, depth = CODES[code]
    n = len(polys)
    pairs = [(n * (2 * D + depth) + 1, n * D + 3), (3, n * (3 * D + depth) - 1), (n * (D + depth), 1)]
    rng = np.random.default_rng(9)
    _, llr = noisy_llrs(rng, K, polys, max(sum(p) for p in pairs) // n + 1)
    x = llr if soft else (llr < 0).astype(np.uint8)
    mem = TorchMemory()
    for pair in pairs:
        model = vm.DecoderModel(K, polys, soft, 8.0, D, depth)
        want = [model.process(x[:pair[0]]), model.process(x[pair[0]:sum(pair)])]
        for in_off in (0, 1):
            for out_off in (0, 1):
                def check(c, got):
                    assert np.array_equal(got, want[c]), (pair, in_off, out_off, c)
                GD.run_guarded(lambda: decoder(K, polys, depth, soft)[0], [x], list(pair), in_off, out_off, mem=mem, call=device_call,
                               max_output=lambda obj, count: obj.max_output(count), in_kind="float" if soft else "bits", out_dtype=np.uint8, out_floats=False,
                               check=check)


def test_guard_words_encoder():
    K, polys, _ = CODES["k7-third"]
    msg = np.random.default_rng(10).integers(0, 2, 800).astype(np.uint8)
    want_all = vm.encode(K, polys, msg)
    mem = TorchMemory()
    for pair in [(513, 3), (3, 255), (256, 1)]:
        want = [want_all[:3 * pair[0]], want_all[3 * pair[0]:3 * sum(pair)]]
        for in_off in (0, 1):
            for out_off in (0, 1):
                def check(c, got):
                    assert np.array_equal(got, want[c]), (pair, in_off, out_off, c)
                GD.run_guarded(lambda: encoder(K, polys), [msg], list(pair), in_off, out_off, mem=mem, call=device_call,
                               max_output=lambda obj, count: obj.max_output(count), in_kind="bits", out_dtype=np.uint8, out_floats=False, check=check)


def test_max_output_is_honoured():
    import torch
    K, polys, _ = CODES["k7"]
    n = len(polys)
    blk, _ = decoder(K, polys)
    for count in (0, 1, 2, n * D - 1, n * D, n * D + 1, 5 * n * D + 3):
        assert blk.max_output(count) == vm.max_output(count, n, D, L)
    x, want = k7_reference()
    take = n * (2 * D + L)
    xt = torch.from_numpy(np.array(x[:take])).cuda()
    yt = torch.zeros(4 * D, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(lr.LrhipError) as e:
        blk.process_device(xt.data_ptr(), take, yt.data_ptr(), 2 * D - 1)
    assert "viterbi: output capacity %d < %d" % (2 * D - 1, 2 * D) in str(e.value)
    # the refused call consumed nothing
    assert blk.process_device(xt.data_ptr(), take, yt.data_ptr(), 2 * D) == 2 * D
    _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
    assert np.array_equal(yt.cpu().numpy()[:2 * D], want[:2 * D])
    enc = encoder(K, polys)
    mt = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(lr.LrhipError) as e:
        enc.process_device(mt.data_ptr(), 10, yt.data_ptr(), 19)
    assert "convenc: output capacity 19 < 20" in str(e.value)


# ---- loopback: bits -> ConvolutionalEncoder -> QuadratureAmplitudeModulator(4) | noise on the host | QuadratureAmplitudeDemodulator(soft) -> ViterbiDecoder
NOISE_VARIANCE = {"clean": 0.05, "noisy": 0.6}


def make(cls, args, in_type, rate=1.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def loopback_blocks(variance):
    K, polys, _ = CODES["k7"]
    tx = [make(lr.ConvolutionalEncoderBlock, [K, polys], types.Bit), make(lr.QuadratureAmplitudeModulatorBlock, [1.0, 1.0, 4], types.Bit, 2.0)]
    rx = [make(lr.QuadratureAmplitudeDemodulatorBlock, [1.0, 1.0, 4, {"soft": True, "noise_variance": variance}], types.ComplexFloat32),
          make(lr.ViterbiDecoderBlock, [K, polys, {"block": D, "depth": L}], types.Float32, 2.0)]
    return tx, rx


def loopback_models(msg, variance, seed):
    """(the samples sent, the samples received, the code bits the LLRs' signs get wrong, the bits the models decode)"""
    K, polys, _ = CODES["k7"]
    table = mm.qam_table(4)
    code = vm.encode(K, polys, msg)
    sent = mm.ModulatorModel(table, 1, True).process(code)
    rng = np.random.default_rng(seed)
    received = (sent + np.sqrt(variance / 2) * (rng.standard_normal(len(sent)) + 1j * rng.standard_normal(len(sent)))).astype(np.complex64)
    llr = dm.DemodulatorModel(table, 1, 0, True, True, np.float32(1.0 / variance), dm.detect_grid(table)).process(received)
    return sent, received, int(np.count_nonzero((llr < 0) != code.astype(bool))), vm.DecoderModel(K, polys, True, 8.0, D, L).process(llr)


@pytest.mark.parametrize("level", list(NOISE_VARIANCE))
def test_loopback_chains(level):
    variance = NOISE_VARIANCE[level]
    msg = np.random.default_rng(12).integers(0, 2, steps(L, windows=8)).astype(np.uint8)
    sent, received, flips, want = loopback_models(msg, variance, 13)
    tx, rx = loopback_blocks(variance)
    tx, rx = lr.Chain(tx), lr.Chain(rx)
    assert tx.in_type is types.Bit and tx.out_type is types.ComplexFloat32 and rx.out_type is types.Bit
    assert np.array_equal(tx.process(msg), sent)
    got = rx.process(received)
    assert len(want) == 8 * D and np.array_equal(got, want)
    errors = int(np.count_nonzero(want != msg[:len(want)]))
    if level == "clean":
        assert errors == 0                                                 # the model gives the message back, hence so does the device
    else:
        assert flips > 20                                                  # the channel did flip code bits


def test_loopback_device_graph():
    variance = NOISE_VARIANCE["clean"]
    K, polys, _ = CODES["k7"]
    msg = np.random.default_rng(14).integers(0, 2, steps(L, windows=6)).astype(np.uint8)
    sent, received, _, want = loopback_models(msg, variance, 15)
    g = lr.DeviceGraph()
    src = g.input("bits", types.Bit, rate=1.0)
    g.connect(src, lr.ConvolutionalEncoderBlock(K, polys), lr.QuadratureAmplitudeModulatorBlock(1.0, 1.0, 4))
    g.initialize()
    (out,) = g.process(bits=msg).values()
    assert np.array_equal(out, sent)
    g = lr.DeviceGraph()
    src = g.input("samples", types.ComplexFloat32, rate=1.0)
    g.connect(src, lr.QuadratureAmplitudeDemodulatorBlock(1.0, 1.0, 4, {"soft": True, "noise_variance": variance}),
              lr.ViterbiDecoderBlock(K, polys, {"block": D, "depth": L}))
    g.initialize()
    (out,) = g.process(samples=received).values()
    assert out.dtype == np.uint8 and np.array_equal(out, want) and np.array_equal(out, msg[:len(out)])


def through_ring(chain, x, sizes):
    """submit / collect: the pieces of x through a ring of three slots; returns the collected parts"""
    chain.set_ring(3, max(sizes))
    parts, pos = [], 0
    for size in sizes:
        if chain.in_flight == 3:
            parts.append(chain.collect())
        chain.submit(x[pos:pos + size])
        pos += size
    while chain.in_flight:
        parts.append(chain.collect())
    assert pos == len(x) and len(parts) == len(sizes)
    return parts


def test_loopback_ring():
    """both chains of the loopback in chunks through a ring of three slots: the message through the encoder and the modulator, then, noise added on the
    host, the received samples through the demodulator and the decoder"""
    variance = NOISE_VARIANCE["noisy"]
    msg = np.random.default_rng(16).integers(0, 2, steps(L, windows=10)).astype(np.uint8)
    sent, received, _, want = loopback_models(msg, variance, 17)
    tx, rx = loopback_blocks(variance)
    sizes = [200, 1, 199, 2, 1, 200]
    sizes.append(len(msg) - sum(sizes))
    assert 0 < sizes[-1] <= 200 and len(received) == len(msg)
    parts = through_ring(lr.Chain(tx), msg, sizes)
    assert [len(p) for p in parts] == sizes and np.array_equal(np.concatenate(parts), sent)
    parts = through_ring(lr.Chain(rx), received, sizes)
    assert any(len(p) == 0 for p in parts)
    assert np.array_equal(np.concatenate(parts), want)


def test_position_counters_refuse_overflow():
    """the counters are 64-bit: a call that would carry the decoder past input 2^64 and a seek that puts the encoder's output there are refused with
    the message, and the refused call changes nothing"""
    K, polys, _ = CODES["k7"]
    n = len(polys)
    top = 1 << 64
    x, _ = k7_reference()
    blk, model = decoder(K, polys)
    n0 = top - n * (D + L) - 5
    blk.seek(n0)
    model.seek(n0)
    first = n * (D + L) - 4
    got, expect = blk.process(x[:first]), model.process(x[:first])                   # up to input 2^64 - 9: the last window there is
    assert len(expect) == D and np.array_equal(got, expect)
    with pytest.raises(lr.LrhipError) as e:
        blk.process(x[first:first + 10])
    assert "viterbi: more than 2^64 input values" in str(e.value)
    assert len(blk.process(x[first:first + 8])) == len(model.process(x[first:first + 8])) == 0      # up to input 2^64 - 1: the refused call consumed nothing
    with pytest.raises(lr.LrhipError) as e:
        blk.process(x[:1])
    assert "viterbi: more than 2^64 input values" in str(e.value)
    enc = encoder(K, polys)
    msg = np.random.default_rng(18).integers(0, 2, 40).astype(np.uint8)
    head = enc.process(msg[:20])
    with pytest.raises(lr.LrhipError) as e:
        enc.seek(top // n)
    assert "convenc: seek to input %d lies behind output 2^64" % (top // n) in str(e.value)
    assert np.array_equal(np.concatenate([head, enc.process(msg[20:])]), vm.encode(K, polys, msg))      # the refused seek forgot nothing
    enc.seek(top // n - 1)
    assert np.array_equal(enc.process(msg), vm.encode(K, polys, msg))
