"""ReedSolomonEncoderBlock, ReedSolomonDecoderBlock, PackBitsBlock and UnpackBitsBlock on the MI355X, byte for byte against the model
(tests/helpers/reedsolomon_model.py).  The parameter sets are where the kernels can go wrong:
    ccsds (255, 223), I = 1   full length, t = 16                      ccsds, I = 5                  stride-5 interleave
    dvb (204, 188)            shortened: roots in the pad are refused   t32 (255, 191)                t = 32, all 64 syndrome lanes
    t1-full (255, 253) and t1-short (10, 8)   t = 1                     n63, n64, n65 (.., n - 16)    one lane stride: below, on and just past 64
    general (255, 239), gfpoly 0x187, fcr 1   another field and root offset
Streams are 37 frames and 5 bytes: no multiple of the waves of a workgroup, and a partial frame stays carried."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, timeshard, types
from tests.helpers import demodulator_models as dm
from tests.helpers import guarded as GD
from tests.helpers import modulator_model as mm
from tests.helpers import reedsolomon_model as rm
from tests.helpers import viterbi_model as vm
from tests.test_gpu_bounds import TorchMemory, device_call

pytestmark = pytest.mark.gpu

SETS = rm.PARAMETER_SETS
CASES = [(name, 1) for name in SETS] + [("ccsds", 5)]
CASE_IDS = ["%s-I%d" % c for c in CASES]
FRAMES, EXTRA = 37, 5


def make(cls, args, in_type, rate=1.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def options(name, I=1, **more):
    return dict(SETS[name][2], interleave=I, **more)


def encoder(name, I=1):
    n, k, _ = SETS[name]
    return make(lr.ReedSolomonEncoderBlock, [n, k, options(name, I)], types.Byte)


def decoder(name, I=1, status=True):
    n, k, _ = SETS[name]
    return make(lr.ReedSolomonDecoderBlock, [n, k, options(name, I, status=status)], types.Byte)


# ---- the streams: one per parameter set, computed once ----------------------------------------------------------------------------------------------
def pad_root_word(rng, short, full):
    """a word of the shortened code whose nearest codeword OF THE FULL-LENGTH CODE, t errors away, is non-zero in the pad: its locator has a root
    there.  A full-length codeword with one non-zero pad byte, that byte taken as received (zero) and t - 1 more errors in real positions"""
    pad, t = full.n - short.n, short.t
    message = [0] * full.k
    message[int(rng.integers(0, pad))] = int(rng.integers(1, 256))
    message[pad:] = [int(v) for v in rng.integers(0, 256, short.k)]
    word = full.encode(message)[pad:]
    for p in rng.choice(short.n, t - 1, replace=False):
        word[p] ^= int(rng.integers(1, 256))
    padded = [0] * pad + word
    out, status = full.decode(padded)
    assert status == t and any(out[:pad])                                   # the full-length decoder corrects it - in the pad
    assert short.decode(word) == (word[:short.k], rm.UNCORRECTABLE)         # which is no position of the shortened code
    return word


def damage(rng, code, word, pattern):
    """one codeword with the error pattern number `pattern`"""
    n, k, t = code.n, code.k, code.t
    word = list(word)

    def hit(positions, values=None):
        for i, p in enumerate(positions):
            word[int(p)] ^= int(rng.integers(1, 256)) if values is None else values[i % len(values)]
    if pattern == 1:
        hit(rng.choice(n, 1))
    elif pattern == 2:
        hit(rng.choice(n, t, replace=False))
    elif pattern == 3:
        hit(rng.choice(n, t + 1, replace=False))
    elif pattern == 4:
        hit(range(n))
    elif pattern == 5:
        hit(k + rng.choice(n - k, t, replace=False))                        # parity only
    elif pattern == 6:
        hit([0, n - 1], [0x5A])                                             # both ends (t = 1, fcr = 0: S_0 = 0, uncorrectable)
    elif pattern == 7:
        hit(rng.choice(n, min(2, t), replace=False), [0x01, 0xFF])
    elif pattern == 8:
        start = int(rng.integers(0, n - t + 1))
        hit(range(start, start + t))                                        # a burst
    return word


_STREAMS = {}


def stream(name, I=1):
    """(message, encoded, received, the model's decoder output with status bytes, the statuses per frame) of 37 frames and 5 bytes"""
    if (name, I) not in _STREAMS:
        n, k, kw = SETS[name]
        code = rm.Code(n, k, **kw)
        rng = np.random.default_rng(1000 * n + 10 * k + I)
        message = rng.integers(0, 256, FRAMES * I * k + EXTRA).astype(np.uint8)
        message[:I * k] = np.arange(I * k) % 256                            # all 256 values occur (k permitting)
        sent = rm.encoder_model(n, k, interleave=I, **kw).process(message)
        assert len(sent) == FRAMES * I * n
        received = sent.copy().reshape(FRAMES, I * n)
        full = rm.Code(255, 255 - (n - k), **kw) if name == "dvb" else None
        for f in range(FRAMES):
            if I > 1 and f % 10 == 9:
                start = int(rng.integers(0, I * n - I * code.t + 1))
                received[f, start:start + I * code.t] ^= rng.integers(1, 256, I * code.t).astype(np.uint8)      # t errors per codeword
                continue
            for c in range(I):
                if full is not None and f % 6 == 5:
                    received[f, c::I] = pad_root_word(rng, code, full)
                else:
                    received[f, c::I] = damage(rng, code, received[f, c::I], (f + c) % 9)
        received = np.concatenate([received.ravel(), rng.integers(0, 256, EXTRA).astype(np.uint8)])
        want = rm.decoder_model(n, k, interleave=I, status=True, **kw).process(received)
        statuses = want.reshape(FRAMES, I * (k + 1))[:, I * k:]
        for a in (message, sent, received, want):
            a.setflags(write=False)
        _STREAMS[(name, I)] = (message, sent, received, want, statuses)
    return _STREAMS[(name, I)]


def without_status(want, name, I):
    n, k, _ = SETS[name]
    return np.ascontiguousarray(want.reshape(FRAMES, I * (k + 1))[:, :I * k]).ravel()


@pytest.mark.parametrize("name,I", CASES, ids=CASE_IDS)
def test_encoder_against_the_model(name, I):
    n, k, _ = SETS[name]
    message, sent, _, _, _ = stream(name, I)
    enc = encoder(name, I)
    got = enc.process(message)
    assert enc.max_output(len(message)) == (FRAMES + 1) * I * n and got.dtype == np.uint8
    assert np.array_equal(got, sent), np.flatnonzero(got != sent)[:8]
    assert len(np.unique(message)) == 256 or k < 200
    assert len(enc.process(message[:I * k - EXTRA])) == I * n              # the five bytes were carried


@pytest.mark.parametrize("status", [True, False], ids=["status", "plain"])
@pytest.mark.parametrize("name,I", CASES, ids=CASE_IDS)
def test_decoder_against_the_model(name, I, status):
    n, k, _ = SETS[name]
    t = (n - k) // 2
    message, _, received, want, statuses = stream(name, I)
    # what the stream holds, on the model's side: clean, corrected up to t and uncorrectable codewords; a miscorrection only where t = 1 admits it
    assert {0, 1, t, rm.UNCORRECTABLE} <= set(statuses.ravel().tolist())
    clean = (statuses != rm.UNCORRECTABLE).all(axis=1)
    assert np.array_equal(want.reshape(FRAMES, -1)[clean, :I * k], message[:FRAMES * I * k].reshape(FRAMES, -1)[clean]) or t == 1
    if I > 1:
        assert (statuses[9::10] == t).all()                                 # the burst of I t bytes is t errors per codeword: corrected
    if name == "dvb":
        assert (statuses[5::6] == rm.UNCORRECTABLE).all() and len(statuses[5::6]) >= 4      # the words with a locator root in the pad
    blk = decoder(name, I, status)
    got = blk.process(received)
    expect = want if status else without_status(want, name, I)
    assert got.dtype == np.uint8 and len(got) == len(expect)
    assert np.array_equal(got, expect), np.flatnonzero(got != expect)[:8]


def cut(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


CHUNKS = ["whole", 1, 7, "F-1", "F", "F+1", "3F+2", "ragged"]


# (one byte per call on the small code alone: 7 500 calls of the shortened DVB code would show nothing more)
@pytest.mark.parametrize("name,I,chunk", [("t1-short", 3, c) for c in CHUNKS] + [("dvb", 1, c) for c in CHUNKS if c != 1],
                         ids=["10-8-I3-%s" % c for c in CHUNKS] + ["dvb-%s" % c for c in CHUNKS if c != 1])
def test_any_chunking_gives_the_same_bytes(name, I, chunk):
    n, k, kw = SETS[name]
    if name == "t1-short":
        rng = np.random.default_rng(31)
        message = rng.integers(0, 256, FRAMES * I * k + EXTRA).astype(np.uint8)
        sent = rm.encoder_model(n, k, interleave=I, **kw).process(message)
        received = sent.copy()
        received[rng.choice(len(sent), len(sent) // 12, replace=False)] ^= 0x40
        want = rm.decoder_model(n, k, interleave=I, status=True, **kw).process(received)
        assert {0, 1, rm.UNCORRECTABLE} <= set(want.reshape(FRAMES, -1)[:, I * k:].ravel().tolist())
    else:
        message, sent, received, want, _ = stream(name, I)
    for blk, x, expect, F in ((encoder(name, I), message, sent, I * k), (decoder(name, I), received, want, I * n)):
        size = {"F-1": F - 1, "F": F, "F+1": F + 1, "3F+2": 3 * F + 2}.get(chunk, chunk)
        sizes = [len(x)] if chunk == "whole" else [0, 5, 0, 0, F - 5, 1, 0, 2 * F, len(x) - 3 * F - 1] if chunk == "ragged" else cut(len(x), size)
        assert sum(sizes) == len(x)
        for _ in range(2):
            parts, pos = [], 0
            for s in sizes:
                got = blk.process(x[pos:pos + s])
                assert len(got) <= blk.max_output(s) and len(got) % blk.frame_out == 0
                parts.append(got)
                pos += s
            got = np.concatenate(parts)
            assert np.array_equal(got, expect), (chunk, len(got), len(expect))
            assert chunk not in (1, 7, "ragged") or any(len(p) == 0 for p in parts)
            blk.reset()                                                     # and the same again


def test_seek_and_time_partitions():
    name = "dvb"
    n, k, kw = SETS[name]
    message, sent, received, want, _ = stream(name)
    for blk, model, x, expect, F, Fo in ((encoder(name), rm.encoder_model(n, k, **kw), message, sent, k, n),
                                         (decoder(name), rm.decoder_model(n, k, status=True, **kw), received, want, n, k + 1)):
        assert blk.memory() == F - 1 == model.memory()
        chain = lr.Chain([blk])
        assert chain.halo() == F - 1 and chain.shard_align() == 1
        fresh = np.random.default_rng(4).integers(0, 256, 3 * F + 3).astype(np.uint8)
        # the block is the model wherever it is started: the bytes of the frame in front of n0 are zeros
        for n0 in (0, 1, F - 1, F, F + 1, 5 * F + 7, (1 << 40) + 3, (1 << 40) * F):
            blk.process(fresh[:9])                                          # another partition's position
            blk.seek(n0)
            model.seek(n0)
            got, wanted = blk.process(fresh), model.process(fresh)
            assert len(wanted) >= 2 * Fo and np.array_equal(got, wanted), n0
        # behind memory() inputs the output is the uninterrupted stream's, at the same absolute positions
        for n0 in (1, F - 1, F, 2 * F + 100, 7 * F + 1):
            blk.seek(n0)
            head = blk.process(x[n0:n0 + F - 1])
            tail = blk.process(x[n0 + F - 1:])
            first = ((n0 + F - 1) // F) * Fo
            assert first == (n0 // F) * Fo + len(head)
            assert len(tail) >= Fo and np.array_equal(tail, expect[first:]), n0
        # cuts on multiples of F are exact without a halo; any other cut replays halo() bytes
        cuts = [0, F, 5 * F, 6 * F, 30 * F, len(x)]
        parts = [timeshard.run_partition(chain, x, a, b, halo=0, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), expect)
        cuts = sorted({0, 1, F - 1, F + 1, 2 * F + 5, 2 * F + 6, 9 * F + 3, 9 * F + 4, len(x)})
        parts = [timeshard.run_partition(chain, x, a, b, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), expect)
        assert len(parts[0]) == 0 and sum(len(p) > 0 for p in parts) >= 4
        for G in (2, 3):
            parts = [timeshard.run_partition(chain, x, a, b) for a, b in timeshard.bounds(len(x), G, align=1)]
            assert np.array_equal(np.concatenate(parts), expect)


@pytest.mark.parametrize("name,I", [("ccsds", 5), ("n65", 1)], ids=["ccsds-I5", "n65"])
def test_pointers_off_16_bytes(name, I):
    import torch
    message, sent, received, want, _ = stream(name, I)
    for blk, x, expect in ((encoder(name, I), message, sent), (decoder(name, I), received, want)):
        for in_off, out_off in ((0, 0), (1, 0), (3, 1), (0, 2), (2, 5), (5, 3)):
            xt = torch.zeros(len(x) + 64, dtype=torch.uint8, device="cuda")
            xt[in_off:in_off + len(x)] = torch.from_numpy(np.array(x)).cuda()
            yt = torch.zeros(len(expect) + 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            blk.reset()
            count = blk.process_device(xt.data_ptr() + in_off, len(x), yt.data_ptr() + out_off, len(expect))
            _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
            raw = yt.cpu().numpy()
            assert count == len(expect) and np.array_equal(raw[out_off:out_off + count], expect), (in_off, out_off)
            assert not raw[:out_off].any() and not raw[out_off + count:].any()


@pytest.mark.parametrize("name,I,which", [("ccsds", 5, "decoder"), ("ccsds", 5, "encoder"), ("n65", 1, "decoder"), ("n65", 1, "encoder"), ("t1-short", 1, "decoder")])
def test_guard_words(name, I, which):
    """tests/helpers/guarded.py, as tests/test_gpu_bounds.py runs it: nothing is written before the output or behind the count, every output of the
    count is written, the input is untouched, and hostile bytes behind the call's n values change nothing"""
    n, k, kw = SETS[name]
    message, sent, received, want, _ = stream(name, I)
    if which == "encoder":
        x, F, factory, model = message, I * k, lambda: encoder(name, I), lambda: rm.encoder_model(n, k, interleave=I, **kw)
    else:
        x, F, factory, model = received, I * n, lambda: decoder(name, I), lambda: rm.decoder_model(n, k, interleave=I, status=True, **kw)
    mem = TorchMemory()
    for pair in [(2 * F + 1, F + 3), (3, 3 * F - 1), (F - 1, 1), (F, 5 * F)]:
        m = model()
        expect = [m.process(x[:pair[0]]), m.process(x[pair[0]:sum(pair)])]
        for in_off, out_off in ((0, 0), (1, 1), (2, 3)):
            def check(c, got):
                assert np.array_equal(got, expect[c]), (pair, in_off, out_off, c)
            GD.run_guarded(factory, [x], list(pair), in_off, out_off, mem=mem, call=device_call, max_output=lambda obj, count: obj.max_output(count),
                           in_kind="raw", out_dtype=np.uint8, out_floats=False, check=check)


def test_max_output_is_honoured_and_tight():
    import torch
    name, I = "ccsds", 5
    n, k, _ = SETS[name]
    F, Fo = I * n, I * (k + 1)
    _, _, received, want, _ = stream(name, I)
    blk = decoder(name, I)
    for count in (0, 1, 2, F - 1, F, F + 1, 5 * F + 3):
        assert blk.max_output(count) == -(-count // F) * Fo
    xt = torch.from_numpy(np.array(received)).cuda()
    yt = torch.zeros(4 * Fo, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert blk.process_device(xt.data_ptr(), F - 1, yt.data_ptr(), 0) == 0
    assert blk.process_device(xt.data_ptr() + F - 1, 1, yt.data_ptr(), blk.max_output(1)) == Fo == blk.max_output(1)       # the bound is reached
    with pytest.raises(lr.LrhipError) as e:
        blk.process_device(xt.data_ptr() + F, 2 * F, yt.data_ptr(), 2 * Fo - 1)
    assert "rsdec: output capacity %d < %d" % (2 * Fo - 1, 2 * Fo) in str(e.value)
    # the refused call consumed nothing
    assert blk.process_device(xt.data_ptr() + F, 2 * F, yt.data_ptr() + Fo, 2 * Fo) == 2 * Fo
    _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
    assert np.array_equal(yt.cpu().numpy()[:3 * Fo], want[:3 * Fo])
    with pytest.raises(lr.LrhipError) as e:
        blk.process_device(None, F, yt.data_ptr(), Fo)
    assert "null buffer" in str(e.value)                                    # (the entry point's refusal; the stage makes its own inside a chain)
    with pytest.raises(lr.LrhipError) as e:
        blk.process_device(xt.data_ptr(), F, None, Fo)
    assert "null buffer" in str(e.value)
    assert blk.process_device(xt.data_ptr() + 3 * F, 3 * F, yt.data_ptr(), 3 * Fo) == 3 * Fo            # the refused calls consumed nothing
    _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
    assert np.array_equal(yt.cpu().numpy()[:3 * Fo], want[3 * Fo:6 * Fo])
    enc = encoder(name, I)
    with pytest.raises(lr.LrhipError) as e:
        enc.process_device(xt.data_ptr(), I * k, yt.data_ptr(), I * n - 1)
    assert "rsenc: output capacity %d < %d" % (I * n - 1, I * n) in str(e.value)
    unpack = make(lr.UnpackBitsBlock, [], types.Byte)
    with pytest.raises(lr.LrhipError) as e:
        unpack.process_device(xt.data_ptr(), (1 << 60) + 1, yt.data_ptr(), 1 << 20)
    assert "unpackbits: more than 2^63 output bytes in one call" in str(e.value)


def test_position_counters_refuse_overflow():
    """the counters are 64-bit: a call that would carry a stage past input 2^64 and a seek that puts the encoder's output there are refused with the
    message, and the refused call changes nothing"""
    name = "t1-short"
    n, k, kw = SETS[name]
    top = 1 << 64
    rng = np.random.default_rng(18)
    x = rng.integers(0, 256, 4 * n).astype(np.uint8)
    blk, model = decoder(name), rm.decoder_model(n, k, status=True, **kw)
    n0 = top - 2 * n - 5
    blk.seek(n0)
    model.seek(n0)
    got, expect = blk.process(x[:n + 3]), model.process(x[:n + 3])
    assert len(expect) == k + 1 and np.array_equal(got, expect)
    with pytest.raises(lr.LrhipError) as e:
        blk.process(x[:n + 2])
    assert "rsdec: more than 2^64 input bytes" in str(e.value)
    got, expect = blk.process(x[:n + 1]), model.process(x[:n + 1])          # up to input 2^64 - 1: the refused call consumed nothing
    assert len(expect) == k + 1 and np.array_equal(got, expect)
    enc = encoder(name)
    message = rng.integers(0, 256, 5 * k).astype(np.uint8)
    head = enc.process(message[:2 * k + 3])
    first_bad = -(-top // n) * k                                            # the first input whose frame count times n reaches 2^64
    with pytest.raises(lr.LrhipError) as e:
        enc.seek(first_bad)
    assert "rsenc: seek to input %d lies behind output 2^64" % first_bad in str(e.value)
    expect = rm.encoder_model(n, k, **kw).process(message)
    assert np.array_equal(np.concatenate([head, enc.process(message[2 * k + 3:])]), expect)       # the refused seek forgot nothing
    enc.seek(first_bad - k)
    assert np.array_equal(enc.process(message), expect)


# ---- bits <-> bytes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["msb", "lsb"])
def test_pack_and_unpack_bits(order):
    msb = order == "msb"
    rng = np.random.default_rng(21)
    bits = rng.integers(0, 256, 8 * 301 + 5).astype(np.uint8)               # junk above bit 0: bit 0 is read
    want = rm.pack((bits & 1)[:8 * 301], msb)
    pack = make(lr.PackBitsBlock, [{"order": order}], types.Bit)
    unpack = make(lr.UnpackBitsBlock, [{"order": order}], types.Byte)
    assert np.array_equal(pack.process(bits), want) and pack.max_output(9) == 2 and pack.max_output(8) == 1 and unpack.max_output(3) == 24
    pack.reset()
    for sizes in (cut(len(bits), 1)[:200], cut(len(bits), 3), cut(len(bits), 7), cut(len(bits), 8), cut(len(bits), 9), [0, 5, 0, 3, 1000, 0, len(bits) - 1008]):
        parts = [pack.process(bits[a:a + s]) for a, s in zip(np.cumsum([0] + sizes[:-1]), sizes)]
        got = np.concatenate(parts)
        assert np.array_equal(got, want[:len(got)]) and len(got) == sum(sizes) // 8
        pack.reset()
    # a seek to a non-multiple of 8 lands on that byte, its bits in front counted as zeros
    model = rm.pack_model(msb)
    for n0 in (0, 3, 8, 13, (1 << 40) + 5):
        pack.seek(n0)
        model.seek(n0)
        assert np.array_equal(pack.process(bits[:100]), model.process(bits[:100] & 1)), n0
    chain = lr.Chain([pack])
    assert chain.halo() == 7
    cuts = [0, 3, 8, 21, 800, 801, len(bits)]
    parts = [timeshard.run_partition(chain, bits, a, b, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), want)
    data = rng.integers(0, 256, 1000).astype(np.uint8)
    got = unpack.process(data)
    assert np.array_equal(got, rm.unpack(data, msb)) and np.array_equal(got, np.unpackbits(data, bitorder="big" if msb else "little"))
    parts = [unpack.process(data[a:b]) for a, b in zip([0, 1, 1, 500], [1, 1, 500, 1000])]
    assert np.array_equal(np.concatenate(parts), got)
    unpack.seek(77)
    assert np.array_equal(unpack.process(data[77:]), got[8 * 77:]) and lr.Chain([unpack]).halo() == 0
    pack.reset()
    assert np.array_equal(pack.process(got), data)                          # the round trip
    mem = TorchMemory()
    for blk_factory, x, kind, model_of in ((lambda: make(lr.PackBitsBlock, [{"order": order}], types.Bit), bits, "bits", lambda: rm.pack_model(msb)),
                                           (lambda: make(lr.UnpackBitsBlock, [{"order": order}], types.Byte), data, "raw", lambda: rm.unpack_model(msb))):
        for pair in [(13, 300), (515, 5)]:
            m = model_of()
            expect = [m.process(x[:pair[0]]), m.process(x[pair[0]:sum(pair)])]
            for in_off, out_off in ((0, 0), (1, 3)):
                def check(c, got):
                    assert np.array_equal(got, expect[c]), (pair, in_off, out_off, c)
                GD.run_guarded(blk_factory, [x], list(pair), in_off, out_off, mem=mem, call=device_call, max_output=lambda obj, count: obj.max_output(count),
                               in_kind=kind, out_dtype=np.uint8, out_floats=False, check=check)


# ---- loopback: bytes -> rsenc -> unpackbits -> convenc -> PAM | noise on the host | soft PAM demodulator -> viterbi -> packbits -> rsdec(status) -----
K, POLYS, D, L = 7, [0o171, 0o133], 256, 48
VARIANCE, LOOP_FRAMES = 0.7, 6


def loopback_blocks():
    n, k, _ = SETS["ccsds"]
    tx = [make(lr.ReedSolomonEncoderBlock, [n, k, options("ccsds")], types.Byte), make(lr.UnpackBitsBlock, [], types.Byte),
          make(lr.ConvolutionalEncoderBlock, [K, POLYS], types.Bit), make(lr.PulseAmplitudeModulatorBlock, [1.0, 1.0, 2], types.Bit)]
    rx = [make(lr.PulseAmplitudeDemodulatorBlock, [1.0, 1.0, 2, {"soft": True, "noise_variance": VARIANCE}], types.Float32),
          make(lr.ViterbiDecoderBlock, [K, POLYS, {"block": D, "depth": L}], types.Float32), make(lr.PackBitsBlock, [], types.Bit),
          make(lr.ReedSolomonDecoderBlock, [n, k, options("ccsds", status=True)], types.Byte)]
    return tx, rx


_LOOP = {}


def loopback_models():
    """(the message, the samples sent, the samples received with the Viterbi decoder's D + L tail of erasures behind them, the model's output):
    noise chosen so that the Viterbi decoder leaves byte errors in at least 4 frames and every codeword stays within t"""
    if not _LOOP:
        n, k, kw = SETS["ccsds"]
        rng = np.random.default_rng(2)
        message = rng.integers(0, 256, LOOP_FRAMES * k).astype(np.uint8)
        coded = rm.encoder_model(n, k, **kw).process(message)
        table = mm.pam_table(2)
        sent = mm.ModulatorModel(table, 1, True).process(vm.encode(K, POLYS, rm.unpack(coded)))
        received = (sent + np.sqrt(VARIANCE) * rng.standard_normal(len(sent))).astype(np.float32)
        received = np.concatenate([received, np.zeros(2 * (D + L), np.float32)])            # n (D + L) erasures: the last bits leave the decoder
        llr = dm.DemodulatorModel(table, 1, 0, True, True, np.float32(1.0 / VARIANCE), None).process(received)
        decided = rm.pack_model().process(vm.DecoderModel(K, POLYS, True, 8.0, D, L).process(llr))
        want = rm.decoder_model(n, k, status=True, **kw).process(decided)
        byte_errors = [int(np.count_nonzero(decided[f * n:(f + 1) * n] != coded[f * n:(f + 1) * n])) for f in range(LOOP_FRAMES)]
        statuses = want.reshape(LOOP_FRAMES, k + 1)[:, k]
        assert sum(e > 0 for e in byte_errors) >= 4 and max(byte_errors) <= (n - k) // 2 and statuses.tolist() == byte_errors
        assert np.array_equal(want.reshape(LOOP_FRAMES, k + 1)[:, :k].ravel(), message)
        for a in (message, sent, received, want):
            a.setflags(write=False)
        _LOOP.update(message=message, sent=sent, received=received, want=want)
    return _LOOP["message"], _LOOP["sent"], _LOOP["received"], _LOOP["want"]


def test_loopback_chains():
    n, k, _ = SETS["ccsds"]
    message, sent, received, want = loopback_models()
    tx, rx = loopback_blocks()
    tx, rx = lr.Chain(tx), lr.Chain(rx)
    assert tx.in_type is types.Byte and tx.out_type is types.Float32 and rx.out_type is types.Byte
    assert np.array_equal(tx.process(message), sent)
    got = rx.process(received)
    assert np.array_equal(got, want) and np.array_equal(got.reshape(LOOP_FRAMES, k + 1)[:, :k].ravel(), message)


def test_loopback_device_graph():
    n, k, _ = SETS["ccsds"]
    message, sent, received, want = loopback_models()
    g = lr.DeviceGraph()
    src = g.input("bytes", types.Byte, rate=1.0)
    g.connect(src, lr.ReedSolomonEncoderBlock(n, k, options("ccsds")), lr.UnpackBitsBlock(), lr.ConvolutionalEncoderBlock(K, POLYS),
              lr.PulseAmplitudeModulatorBlock(1.0, 1.0, 2))
    g.initialize()
    (out,) = g.process(bytes=message).values()
    assert np.array_equal(out, sent)
    g = lr.DeviceGraph()
    src = g.input("samples", types.Float32, rate=1.0)
    g.connect(src, lr.PulseAmplitudeDemodulatorBlock(1.0, 1.0, 2, {"soft": True, "noise_variance": VARIANCE}),
              lr.ViterbiDecoderBlock(K, POLYS, {"block": D, "depth": L}), lr.PackBitsBlock(), lr.ReedSolomonDecoderBlock(n, k, options("ccsds", status=True)))
    g.initialize()
    (out,) = g.process(samples=received).values()
    assert out.dtype == np.uint8 and np.array_equal(out, want)


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
    message, sent, received, want = loopback_models()
    tx, rx = loopback_blocks()
    sizes = [200, 1, 199, 23, 400]
    sizes.append(len(message) - sum(sizes))
    parts = through_ring(lr.Chain(tx), message, sizes)
    assert any(len(p) == 0 for p in parts) and np.array_equal(np.concatenate(parts), sent)
    sizes = [5000, 1, 4999, 2, 8000]
    sizes.append(len(received) - sum(sizes))
    assert sizes[-1] > 0
    parts = through_ring(lr.Chain(rx), received, sizes)
    assert any(len(p) == 0 for p in parts) and np.array_equal(np.concatenate(parts), want)
