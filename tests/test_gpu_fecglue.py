"""PunctureBlock, DepunctureBlock, ConvolutionalInterleaverBlock, ConvolutionalDeinterleaverBlock, AdditiveScramblerBlock and the DVB-S FEC chains on
the MI355X, byte for byte against the models (tests/helpers/fecglue_model.py).  The shapes are where the kernels can go wrong: patterns of one kept
element in 64 at either end, streams that leave a partial frame carried and streams long enough for several workgroups, interleavers of depth 2 and
of depth 61 440 (a tile with a halo larger than itself), calls shorter than the carried depth, tables shorter than a 16-byte word, and pointers at
every offset within one."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, timeshard, types
from tests.helpers import fecglue_model as fm
from tests.helpers import guarded as GD
from tests.test_gpu_bounds import TorchMemory, device_call

pytestmark = pytest.mark.gpu

PATTERNS = list(fm.DVBS_PUNCTURE.values()) + ["10", "0" * 63 + "1", "1" + "0" * 63]
SHAPES = [(2, 1), (3, 5), (12, 17), (52, 4), (16, 256), (256, 1)]
FRAMES, EXTRA, LONG = 37, 5, 20000


def make(cls, args, in_type, rate=1.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def cut(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def in_pieces(blk, x, sizes):
    assert sum(sizes) == len(x)
    parts, pos = [], 0
    for s in sizes:
        got = blk.process(x[pos:pos + s])
        assert len(got) <= blk.max_output(s)
        parts.append(got)
        pos += s
    return parts


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- puncture / depuncture --------------------------------------------------------------------------------------------------------------------------
KINDS = {"puncture": (lambda p: make(lr.PunctureBlock, [p], types.Bit), lambda p: fm.puncture_model(p), np.uint8),
         "llr": (lambda p: make(lr.DepunctureBlock, [p], types.Float32), lambda p: fm.depuncture_model(p, True), np.float32),
         "bit": (lambda p: make(lr.DepunctureBlock, [p, {"soft": False}], types.Bit), lambda p: fm.depuncture_model(p, False), np.uint8)}


def framed_input(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "llr":
        x = (4.0 * rng.standard_normal(n)).astype(np.float32)
        x.view(np.uint32)[3] = 0x7FC12345                           # a NaN with a payload
        x.view(np.uint32)[4] = 0xFFC00001
        x.view(np.uint32)[6] = 0x80000000                           # -0.0
        return x
    return rng.integers(0, 256, n).astype(np.uint8) if kind == "bit" else rng.integers(0, 2, n).astype(np.uint8)


@pytest.mark.parametrize("pattern", PATTERNS, ids=["p%d-%d" % (len(p), p.count("1")) + ("-first" if p[0] == "1" and len(p) == 64 else "") for p in PATTERNS])
@pytest.mark.parametrize("kind", list(KINDS))
def test_puncture_and_depuncture_against_the_model(kind, pattern):
    factory, model_of, _ = KINDS[kind]
    blk, model = factory(pattern), model_of(pattern)
    fi, fo = model.fi, model.fo
    assert (blk.frame_in, blk.frame_out) == (fi, fo)
    short, long_ = framed_input(kind, FRAMES * fi + EXTRA, 1), framed_input(kind, LONG + 3, 2)
    for x, chunks in ((short, (1, 7, 64)), (long_, (7, 64, 4099))):
        want = model_of(pattern).process(x)
        assert len(want) == (len(x) // fi) * fo
        got = blk.process(x)
        assert blk.max_output(len(x)) == -(-len(x) // fi) * fo and same_bytes(got, want), np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))[:8]
        for chunk in chunks:
            blk.reset()
            parts = in_pieces(blk, x, cut(len(x), chunk))
            assert same_bytes(np.concatenate(parts), want), chunk
            assert chunk >= fi or any(len(p) == 0 for p in parts)   # calls that complete no frame
            assert all(len(p) % fo == 0 for p in parts)
        blk.reset()
    if kind == "llr":
        keep = [j for j, c in enumerate(pattern) if c == "1"]
        bits = blk.process(short).view(np.uint32)
        where = {e: (e // fi) * fo + keep[e % fi] for e in (3, 4, 6)}
        assert [int(bits[where[e]]) for e in (3, 4, 6)] == [0x7FC12345, 0xFFC00001, 0x80000000]
        assert not bits[[j for j, c in enumerate(pattern) if c == "0"]].any()             # +0.0, not -0.0


# ---- interleaver and deinterleaver ------------------------------------------------------------------------------------------------------------------
_INTER = {}


def interleaver_stream(I, M, deinterleave):
    """(input, the literal model's output of one call) of 2 D + 12 365 bytes"""
    key = (I, M, deinterleave)
    if key not in _INTER:
        D = (I - 1) * M * I
        x = np.random.default_rng(100 * I + M).integers(0, 256, 2 * D + 12365).astype(np.uint8)
        want = fm.ConvolutionalInterleaverModel(I, M, deinterleave).process(x)
        assert np.array_equal(want, fm.interleave_fast(x, I, M, deinterleave))
        x.setflags(write=False)
        want.setflags(write=False)
        _INTER[key] = (x, want)
    return _INTER[key]


def interleaver(I, M, deinterleave):
    return make(lr.ConvolutionalDeinterleaverBlock if deinterleave else lr.ConvolutionalInterleaverBlock, [I, M], types.Byte)


@pytest.mark.parametrize("deinterleave", [False, True], ids=["interleave", "deinterleave"])
@pytest.mark.parametrize("I,M", SHAPES)
def test_interleavers_against_the_model(I, M, deinterleave):
    D = (I - 1) * M * I
    x, want = interleaver_stream(I, M, deinterleave)
    blk = interleaver(I, M, deinterleave)
    assert blk.memory() == D and blk.max_output(len(x)) == len(x)
    got = blk.process(x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    first = max(1, D - 1)                                           # a first call shorter than D, one byte, a call longer than D, the rest in two
    for sizes in ([first, 1, D + 5, 4099, len(x) - first - D - 4105], [1, 1, 0, 2, D, D + 1, len(x) - 2 * D - 5], cut(len(x), 4099)):
        blk.reset()
        assert min(sizes) >= 0 and np.array_equal(np.concatenate(in_pieces(blk, x, sizes)), want), sizes[:6]
    if not deinterleave:
        back = interleaver(I, M, True).process(got)
        assert not back[:D].any() and np.array_equal(back[D:], x[:len(x) - D])       # the pair is a delay of D


# ---- scrambler --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 7, 255, 1504, 8192])
def test_scrambler_against_the_model(P):
    rng = np.random.default_rng(P)
    table = lr.dvb_energy_dispersal_table() if P == 1504 else rng.integers(0, 256, P).astype(np.uint8)
    x = rng.integers(0, 256, 20011).astype(np.uint8)
    for K in sorted({0, P - 1}):
        want = fm.ScramblerModel(table, K).process(x)
        assert np.array_equal(want, fm.scramble_fast(x, table, K))
        blk = make(lr.AdditiveScramblerBlock, [table, {"offset": K}], types.Byte)
        assert np.array_equal(blk.process(x), want) and blk.max_output(77) == 77 and blk.memory() == 0
        for sizes in ([1, 12, 4086, len(x) - 4099], cut(len(x), 13), cut(len(x), 4099), [1] * 3100 + [len(x) - 3100]):
            blk.reset()
            assert np.array_equal(np.concatenate(in_pieces(blk, x, sizes)), want), (K, sizes[:3])
        blk.reset()
        assert np.array_equal(blk.process(want), x)                 # the same block descrambles


# ---- every stage: seek, time partitions, pointers, guards, max_output -------------------------------------------------------------------------------
TABLE7 = np.array([0x5A, 0x01, 0xFF, 0x00, 0x80, 0x33, 0xC4], np.uint8)
STAGES = {
    "puncture": (lambda: make(lr.PunctureBlock, ["1101100110"], types.Bit), lambda: fm.puncture_model("1101100110"), "bits"),
    "depuncture-llr": (lambda: make(lr.DepunctureBlock, ["11010101100110"], types.Float32), lambda: fm.depuncture_model("11010101100110"), "float"),
    "depuncture-bit": (lambda: make(lr.DepunctureBlock, ["110110", {"soft": False}], types.Bit), lambda: fm.depuncture_model("110110", False), "bits"),
    "convinterleave": (lambda: interleaver(12, 17, False), lambda: fm.ConvolutionalInterleaverModel(12, 17), "raw"),
    "convdeinterleave": (lambda: interleaver(3, 5, True), lambda: fm.ConvolutionalInterleaverModel(3, 5, True), "raw"),
    "convinterleave-deep": (lambda: interleaver(16, 256, False), lambda: fm.ConvolutionalInterleaverModel(16, 256), "raw"),
    "scrambler": (lambda: make(lr.AdditiveScramblerBlock, [lr.dvb_energy_dispersal_table(189), {"offset": 945}], types.Byte),
                  lambda: fm.ScramblerModel(fm.dvb_energy_dispersal_table(189), 945), "raw"),
    "scrambler-7": (lambda: make(lr.AdditiveScramblerBlock, [TABLE7, {"offset": 6}], types.Byte), lambda: fm.ScramblerModel(TABLE7, 6), "raw"),
}


def stage_input(name, n, seed=9):
    rng = np.random.default_rng(seed)
    kind = STAGES[name][2]
    return rng.uniform(-8, 8, n).astype(np.float32) if kind == "float" else rng.integers(0, 2 if name == "puncture" else 256, n).astype(np.uint8)


@pytest.mark.parametrize("name", list(STAGES))
def test_seek_and_time_partitions(name):
    factory, model_of, _ = STAGES[name]
    blk, model = factory(), model_of()
    memory = model.memory()
    assert blk.memory() == memory
    chain = lr.Chain([blk])
    assert chain.halo() == memory and chain.shard_align() == 1
    fi, fo = (model.fi, model.fo) if isinstance(model, fm.FramedModel) else (1, 1)
    n = 3 * memory + 4000 if memory < 20000 else 2 * memory + 9000
    x = stage_input(name, n)
    expect = model_of().process(x)
    # the block is the model wherever it is started: everything in front of n0 counts as zeros
    fresh = stage_input(name, min(n, memory + 300), 10)
    # (the frame stages refuse a seek whose OUTPUT position lies behind 2^64, as the Reed-Solomon stages do: theirs stops at 2^62)
    for n0 in (0, 1, fi, 5 * fi + 7, (1 << 40) + 3, (1 << 62) + 5 if fi > 1 else (1 << 64) - len(fresh) - 1):
        blk.process(fresh[:9])                                      # another partition's position
        blk.seek(n0)
        model.seek(n0)
        got, wanted = blk.process(fresh), model.process(fresh)
        assert len(wanted) >= 2 * fo and same_bytes(got, wanted), n0
    # behind memory() inputs the output is the uninterrupted stream's, at the same absolute positions
    for n0 in (1, fi + 1, 2 * fi + 100, 997):
        blk.seek(n0)
        head = blk.process(x[n0:n0 + memory])
        tail = blk.process(x[n0 + memory:])
        first = ((n0 + memory) // fi) * fo
        assert first == (n0 // fi) * fo + len(head)
        assert len(tail) >= fo and same_bytes(tail, expect[first:]), n0
    # cuts on multiples of the frame are exact without a halo only where nothing is carried across them; any cut replays halo() inputs
    cuts = sorted({0, 1, fi + 1, 2 * fi + 5, 2 * fi + 6, 1000, 1001, memory + 1500, len(x)})
    parts = [timeshard.run_partition(chain, x, a, b, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
    assert same_bytes(np.concatenate(parts), expect)
    if fi == 1 and memory == 0:
        parts = [timeshard.run_partition(chain, x, a, b, halo=0, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
        assert same_bytes(np.concatenate(parts), expect)
    for G in (2, 3):
        parts = [timeshard.run_partition(chain, x, a, b) for a, b in timeshard.bounds(len(x), G, align=1)]
        assert same_bytes(np.concatenate(parts), expect)


@pytest.mark.parametrize("name", list(STAGES))
def test_pointers_off_16_bytes(name):
    import torch
    factory, model_of, kind = STAGES[name]
    blk = factory()
    x = stage_input(name, 5000 if "deep" not in name else 70000)
    expect = model_of().process(x)
    es_in, es_out = x.dtype.itemsize, expect.dtype.itemsize
    for in_off, out_off in ((0, 0), (1, 0), (3, 1), (0, 3), (1, 3), (5, 15), (15, 2)):
        xt = torch.zeros(len(x) * es_in + 256, dtype=torch.uint8, device="cuda")
        xt[in_off * es_in:in_off * es_in + len(x) * es_in] = torch.from_numpy(np.array(x).view(np.uint8)).cuda()
        yt = torch.zeros(len(expect) * es_out + 256, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        blk.reset()
        count = blk.process_device(xt.data_ptr() + in_off * es_in, len(x), yt.data_ptr() + out_off * es_out, len(expect))
        _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
        raw = yt.cpu().numpy()
        lo, hi = out_off * es_out, (out_off + count) * es_out
        assert count == len(expect) and np.array_equal(raw[lo:hi], expect.view(np.uint8)), (in_off, out_off)
        assert not raw[:lo].any() and not raw[hi:].any()


@pytest.mark.parametrize("name", list(STAGES))
def test_guard_words(name):
    """tests/helpers/guarded.py, as tests/test_gpu_bounds.py runs it: nothing is written before the output or behind the count, every output of the
    count is written, the input is untouched, and hostile bytes behind the call's n values change nothing"""
    factory, model_of, kind = STAGES[name]
    model = model_of()
    memory = model.memory()
    fi = model.fi if isinstance(model, fm.FramedModel) else 1
    x = stage_input(name, 2 * memory + 9000)
    mem = TorchMemory()
    out_dtype = np.float32 if name.startswith("depuncture") else np.uint8
    for pair in [(2 * fi + 1, fi + 3), (3, 3 * fi - 1 if fi > 1 else 40), (max(1, memory - 1), 1), (memory + 17, 4099)]:
        m = model_of()
        expect = [m.process(x[:pair[0]]), m.process(x[pair[0]:sum(pair)])]
        for in_off, out_off in ((0, 0), (1, 1), (2, 3)):
            def check(c, got):
                assert same_bytes(got, expect[c]), (pair, in_off, out_off, c)
            GD.run_guarded(factory, [x], list(pair), in_off, out_off, mem=mem, call=device_call, max_output=lambda obj, count: obj.max_output(count),
                           in_kind=kind, out_dtype=out_dtype, out_floats=out_dtype == np.float32, check=check)


def test_max_output_is_honoured_and_tight():
    import torch
    xt = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    yt = torch.zeros(1 << 18, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for name, who in (("puncture", "puncture"), ("depuncture-llr", "depuncture"), ("depuncture-bit", "depuncture")):
        blk, model = STAGES[name][0](), STAGES[name][1]()
        fi, fo = model.fi, model.fo
        for count in (0, 1, 2, fi - 1, fi, fi + 1, 5 * fi + 3):
            assert blk.max_output(count) == -(-count // fi) * fo
        assert blk.process_device(xt.data_ptr(), fi - 1, yt.data_ptr(), 0) == 0
        assert blk.process_device(xt.data_ptr(), 1, yt.data_ptr(), blk.max_output(1)) == fo == blk.max_output(1)          # the bound is reached
        with pytest.raises(lr.LrhipError) as e:
            blk.process_device(xt.data_ptr(), 2 * fi, yt.data_ptr(), 2 * fo - 1)
        assert "%s: output capacity %d < %d" % (who, 2 * fo - 1, 2 * fo) in str(e.value)
        assert blk.process_device(xt.data_ptr(), 2 * fi, yt.data_ptr(), 2 * fo) == 2 * fo                                  # the refused call consumed nothing
    for name, who in (("convinterleave", "convinterleave"), ("convdeinterleave", "convdeinterleave"), ("scrambler", "scrambler")):
        blk = STAGES[name][0]()
        assert [blk.max_output(c) for c in (0, 1, 4099)] == [0, 1, 4099]
        with pytest.raises(lr.LrhipError) as e:
            blk.process_device(xt.data_ptr(), 100, yt.data_ptr(), 99)
        assert "%s: output capacity 99 < 100" % who in str(e.value)
        assert blk.process_device(xt.data_ptr(), 100, yt.data_ptr(), 100) == 100
    _lib.check(_lib.load().lrhip_synchronize(), "synchronize")


# ---- DVB-S loopback ---------------------------------------------------------------------------------------------------------------------------------
PACKETS, FILL = 24, fm.DVBS_FILL_PACKETS
BLOCK = 512
VARIANCE, NOISE_SEED, NOISY_RATE, NOISY_DEPTH = 0.30, 1, "3/4", 48
_DVB = {}


def dvb_message():
    """(35 transport packets, the model's scrambled and Reed-Solomon coded packets, the model's interleaved and convolutionally coded bits)"""
    if "message" not in _DVB:
        packets = fm.ts_packets(np.random.default_rng(11), PACKETS + FILL)
        models = fm.dvbs_encoder_model("1/2").models
        coded = models[1].process(models[0].process(packets))
        bits = models[4].process(models[3].process(models[2].process(coded)))
        for a in (packets, coded, bits):
            a.setflags(write=False)
        _DVB["message"] = (packets, coded, bits)
    return _DVB["message"]


def demodulator(variance):
    return make(lr.PulseAmplitudeDemodulatorBlock, [1.0, 1.0, 2, {"soft": True, "noise_variance": variance}], types.Float32)


@pytest.mark.parametrize("rate", list(fm.DVBS_PUNCTURE))
def test_dvbs_loopback_clean(rate):
    packets, _, bits = dvb_message()
    tx = lr.dvbs_fec_encoder(rate)
    assert tx.in_type is types.Byte and tx.out_type is types.Bit
    sent_bits = tx.process(packets)
    assert np.array_equal(sent_bits, fm.puncture_model(fm.DVBS_PUNCTURE[rate]).process(bits))
    depth = lr.DVBS_DEPTH[rate]
    samples = np.concatenate([fm.pam2(sent_bits), np.zeros(2 * (BLOCK + depth), np.float32)])          # erasures for the Viterbi tail
    rx = lr.dvbs_fec_decoder(rate)
    assert rx.in_type is types.Float32 and rx.out_type is types.Byte
    out = rx.process(demodulator(1.0).process(samples))
    assert len(out) == (PACKETS + FILL) * 188
    assert np.array_equal(out[FILL * 188:], packets[:PACKETS * 188])
    # hard decisions, with the status bytes
    hard = lr.dvbs_fec_decoder(rate, soft=False, status=True)
    tail = np.zeros(2 * (BLOCK + depth), np.uint8)
    out = hard.process(np.concatenate([sent_bits, tail]))
    frames = out[:len(out) // 189 * 189].reshape(-1, 189)
    assert len(frames) >= FILL + PACKETS - 1                        # the tail is bits, not erasures: the last packet may be hit
    assert np.array_equal(frames[FILL:FILL + PACKETS - 1, :188].ravel(), packets[:(PACKETS - 1) * 188]) and not frames[FILL:FILL + PACKETS - 1, 188].any()


def noisy_models():
    """(the samples received, with the erasures of the Viterbi tail behind them; the model's output with status bytes): noise chosen so that the
    Viterbi model leaves byte errors in at least 4 of the 24 codewords behind the deinterleaver and every codeword stays within t = 8"""
    if "noisy" not in _DVB:
        packets, coded, bits = dvb_message()
        sent = fm.pam2(fm.puncture_model(fm.DVBS_PUNCTURE[NOISY_RATE]).process(bits))
        rng = np.random.default_rng(NOISE_SEED)
        received = (sent + np.sqrt(VARIANCE) * rng.standard_normal(len(sent))).astype(np.float32)
        received = np.concatenate([received, np.zeros(2 * (BLOCK + NOISY_DEPTH), np.float32)])
        x = fm.pam2_llrs(received, VARIANCE)
        stages = fm.dvbs_decoder_stages(NOISY_RATE, True, True, BLOCK, NOISY_DEPTH)
        for m in stages[:4]:
            x = m.process(x)
        words = x[:(FILL + PACKETS) * 204].reshape(-1, 204)[FILL:]
        byte_errors = [int(np.count_nonzero(words[f] != coded[f * 204:(f + 1) * 204])) for f in range(PACKETS)]
        want = stages[5].process(stages[4].process(x))
        frames = want.reshape(-1, 189)
        assert len(frames) == FILL + PACKETS
        statuses = frames[FILL:, 188]
        assert sum(e > 0 for e in byte_errors) >= 4 and max(byte_errors) <= 8 and statuses.tolist() == byte_errors, byte_errors
        assert np.array_equal(frames[FILL:, :188].ravel(), packets[:PACKETS * 188])
        received.setflags(write=False)
        want.setflags(write=False)
        _DVB["noisy"] = (received, want)
    return _DVB["noisy"]


def noisy_blocks():
    return [lr.PulseAmplitudeDemodulatorBlock(1.0, 1.0, 2, {"soft": True, "noise_variance": VARIANCE})] + lr.dvbs_fec_decoder_blocks(
        NOISY_RATE, status=True, block=BLOCK, depth=NOISY_DEPTH)


def noisy_chain():
    blocks, rate, t = noisy_blocks(), 1.0, [types.Float32]
    for b in blocks:
        b.rate = rate
        b.differentiate(t)
        b.initialize()
        rate, t = b.get_rate(), [b.get_output_type()]
    return lr.Chain(blocks)


def test_dvbs_loopback_noisy_chain():
    received, want = noisy_models()
    chain = noisy_chain()
    assert chain.out_type is types.Byte
    got = chain.process(received)
    assert np.array_equal(got, want), np.flatnonzero(got[:len(want)] != want[:len(got)])[:8]
    # the decoder of composites.py alone, behind the demodulator block
    rx = lr.dvbs_fec_decoder(NOISY_RATE, status=True, block=BLOCK, depth=NOISY_DEPTH)
    assert np.array_equal(rx.process(demodulator(VARIANCE).process(received)), want)


def test_dvbs_loopback_noisy_device_graph():
    received, want = noisy_models()
    g = lr.DeviceGraph()
    src = g.input("samples", types.Float32, rate=1.0)
    g.connect(src, *noisy_blocks())
    g.initialize()
    (out,) = g.process(samples=received).values()
    assert out.dtype == np.uint8 and np.array_equal(out, want)


def test_dvbs_loopback_noisy_ring():
    received, want = noisy_models()
    chain = noisy_chain()
    sizes = [5000, 1, 4999, 2, 30000, 7]
    sizes.append(len(received) - sum(sizes))
    assert sizes[-1] > 0
    chain.set_ring(3, max(sizes))
    parts, pos = [], 0
    for size in sizes:
        if chain.in_flight == 3:
            parts.append(chain.collect())
        chain.submit(received[pos:pos + size])
        pos += size
    while chain.in_flight:
        parts.append(chain.collect())
    assert len(parts) == len(sizes) and any(len(p) == 0 for p in parts) and np.array_equal(np.concatenate(parts), want)
