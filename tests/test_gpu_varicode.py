"""VaricodeDecoderBlock and bpsk31_receiver(decoder=True) on the MI355X, character for character against the literal loop
(tests/helpers/varicode_model.py): the reference's golden vectors, random streams whole and in ragged calls (every call's output, not only
the concatenation) at the sizes where the kernels change path, runs of ones over tile and call boundaries, every character of the alphabet,
bytes other than 0 and 1, a text, reset(), the bookkeeping, and the receiver end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import digital_signals as ds
from tests.helpers import varicode_model as vm

pytestmark = pytest.mark.gpu

TILE = 4096                                              # DG_TILE: 256 threads x 16 bytes
# the state limit and a thread's chunk; a tile; three tiles with the most carried; more tiles than the carry workgroup has threads
LENGTHS = [1, 2, 3, 10, 11, 12, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 10, 257 * TILE + 5]


def decoder():
    blk = lr.VaricodeDecoderBlock()
    blk.differentiate([types.Bit])
    blk.initialize()
    return blk


def text_of(y):
    return bytes(np.asarray(y, np.uint8))


def literal(x):
    """the literal loop over the whole of x, once: (characters, the index of the byte that completed each).  The loop does not see where the
    calls are cut (tests/test_varicode_cpu.py holds it to that), so a call [a, b) owes the characters with a <= index < b."""
    lit = vm.VaricodeLiteral()
    chars = lit.process(x)
    return chars, np.array(lit.positions, np.int64)


def assert_calls_equal(blk, ref, x, edges):
    """every call's output equals the literal loop's, and stays under the block's bound"""
    chars, at = ref
    for a, b in zip(edges[:-1], edges[1:]):
        got, want = blk.process(x[a:b]), chars[np.searchsorted(at, a):np.searchsorted(at, b)]
        assert got.dtype == np.uint8 and len(got) <= blk.max_output(b - a)
        assert np.array_equal(got, want), (a, b, len(got), len(want))


def ragged(n, seed, most):
    """call boundaries: lengths 1 .. most, drawn until n is used up"""
    rng = np.random.default_rng(seed)
    edges = [0]
    while edges[-1] < n:
        edges.append(min(n, edges[-1] + int(rng.integers(1, most + 1))))
    return edges


@functools.lru_cache(maxsize=None)
def stream(n, p1):
    """random bits with P(1) = p1, and their reference"""
    x = (np.random.default_rng(n + int(10 * p1)).random(n) < p1).astype(np.uint8)
    return x, literal(x)


# ---- golden vectors ------------------------------------------------------------------------------------------------------------------
def test_golden_varicodedecoder():
    vectors = golden_util.load("varicodedecoder_spec")["vectors"]
    assert len(vectors) == 3
    for v in vectors:
        x, want = np.asarray(v["inputs"][0], np.uint8), np.asarray(v["outputs"][0], np.uint8)
        whole, samplewise = golden_util.run_whole_and_samplewise(decoder, x)
        assert whole.dtype == np.uint8
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)
    assert text_of(decoder().process(np.asarray(vectors[0]["inputs"][0], np.uint8))) == b"Hello World"


# ---- random streams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p1", [0.5, 0.3])
@pytest.mark.parametrize("n", LENGTHS)
def test_random_streams_whole_and_ragged(n, p1):
    x, ref = stream(n, p1)
    blk = decoder()
    assert_calls_equal(blk, ref, x, [0, n])
    if n >= TILE:
        assert len(ref[0]) >= n // 20                    # the comparison is not empty (0.117 and 0.144 characters per bit on the CPU)
    # three sets of ragged cuts into the same block: calls of a few bytes (the carried state at every length), of about a tile, and of several tiles
    # (of the longest stream only its first three tiles go through the few-byte calls: 10 000 calls)
    for k, most in enumerate((7 if n <= 3 * TILE else 0, TILE + TILE // 2, 100 * TILE)):
        blk.reset()
        if most:
            assert_calls_equal(blk, ref, x, ragged(n, 31 * n + k, most))
        else:
            assert_calls_equal(blk, ref, x, ragged(2 * TILE + 10, 31 * n + k, 7)[:-1] + [n])


def test_bytes_other_than_zero_and_one():
    """2 % of 2, 128 and 255: such a byte is neither a delimiter zero nor a one"""
    n = 3 * TILE + 77
    rng = np.random.default_rng(12)
    x = (rng.random(n) < 0.5).astype(np.uint8)
    odd = rng.random(n) < 0.02
    x[odd] = rng.choice(np.array([2, 128, 255], np.uint8), int(odd.sum()))
    ref = literal(x)
    # they matter: read as their lowest bit, or as ones, the stream decodes differently
    assert 40 < odd.sum() and len(ref[0]) > n // 20
    assert not np.array_equal(ref[0], literal(x & 1)[0]) and not np.array_equal(ref[0], literal((x != 0).astype(np.uint8))[0])
    blk = decoder()
    assert_calls_equal(blk, ref, x, [0, n])
    blk.reset()
    assert_calls_equal(blk, ref, x, ragged(n, 5, 300))


# ---- runs of ones --------------------------------------------------------------------------------------------------------------------
def test_runs_of_ones_over_a_tile_boundary_and_a_call_cut():
    """R ones, then a character and 00, the run straddling the boundary between two tiles of one call, then the same across a call cut: on a
    run of ones the entry states do not converge, so the character's fate depends on a state composed across the boundary"""
    fates = set()
    blk = decoder()
    for R in range(24):
        head = np.zeros(TILE - (R + 1) // 2, np.uint8)   # the run lies on bytes TILE - (R + 1) / 2 .. TILE + R / 2 - 1
        head[100:TILE - 100:3] = 1                       # (1 0 0)*, spaces: the tile in front is not empty either
        x = np.concatenate([head, np.ones(R, np.uint8), vm.encode("e", lead=0), vm.encode("t", lead=0), vm.encode("hello", lead=0)])
        want = vm.VaricodeLiteral().process(x)
        fates.add(text_of(want).lstrip(b" "))
        blk.reset()
        assert np.array_equal(blk.process(x), want), R
        for cut in sorted({len(head), TILE, len(head) + R, len(head) + R + 1}):
            blk.reset()
            got = np.concatenate([blk.process(x[:cut]), blk.process(x[cut:])])
            assert np.array_equal(got, want), (R, cut)
    # emitted as it is, lost, and merged with the ones into another character
    assert b"ethello" in fates and b"thello" in fates and len(fates) >= 8


# ---- the alphabet --------------------------------------------------------------------------------------------------------------------
def test_every_character_between_a_delimiter_and_an_e():
    x = np.concatenate([vm.encode([c, ord("e")], lead=2) for c in range(128)])
    want = vm.VaricodeLiteral().process(x)
    assert len(want) == 128 + 88 and set(range(128)) - set(want.tolist()) == set(vm.TEN_BIT)
    blk = decoder()
    assert np.array_equal(blk.process(x), want)
    for c in range(128):                                 # and one by one, from an empty state
        blk.reset()
        got = text_of(blk.process(vm.encode([c, ord("e")], lead=2)))
        assert got == (b"e" if c in vm.TEN_BIT else bytes([c]) + b"e"), (c, got)
    blk.reset()
    assert text_of(blk.process(vm.encode("!Zx"))) == b"!x"
    blk.reset()
    assert text_of(blk.process(vm.encode("CQ de Zulu?"))) == b"CQ de ulu"


def test_a_text_comes_back_exactly():
    """0 .. 5 extra idle zeros between the characters.  An odd number of them leaves one zero in the state, which costs the next character a
    bit of room, so the text is drawn from the 54 characters whose codes have at most 8 bits: those come back whatever the idling."""
    rng = np.random.default_rng(8)
    decodable = np.array([c for c in range(128) if vm.CODE[c] < 0x100], np.uint8)
    assert len(decodable) == 54 and set(b"de test 0123 pse k") <= set(decodable.tolist())
    text = rng.choice(decodable, 3000)
    x = vm.encode(text.tolist(), idle=rng.integers(0, 6, len(text)).tolist())
    assert len(x) > 5 * TILE and np.array_equal(vm.VaricodeLiteral().process(x), text)
    blk = decoder()
    assert np.array_equal(blk.process(x), text)
    blk.reset()
    edges = ragged(len(x), 9, 2000)
    assert np.array_equal(np.concatenate([blk.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]), text)


# ---- state and bookkeeping -----------------------------------------------------------------------------------------------------------
def test_reset_in_the_middle_of_a_character_drops_the_state():
    x = vm.encode("hello")
    cut = 2 + 3                                          # three bits into the h (101011)
    blk = decoder()
    assert len(blk.process(x[:cut])) == 0
    assert text_of(blk.process(x[cut:])) == b"hello"
    blk.reset()
    assert len(blk.process(x[:cut])) == 0
    blk.reset()
    want = vm.VaricodeLiteral().process(x[cut:])         # 0 11 00 ...: an `e` where the h was
    assert text_of(want) == b"eello" and np.array_equal(blk.process(x[cut:]), want)


def test_bookkeeping():
    L = _lib.load()
    blk = decoder()
    assert blk.get_output_type() is types.Byte
    assert [blk.max_output(n) for n in (0, 1, 2, 3, 5, 6, 100, 4096)] == [vm.max_output(n) for n in (0, 1, 2, 3, 5, 6, 100, 4096)]
    assert blk.max_output(100) == 36 and blk.max_output(2) == 2
    assert len(blk.process(np.zeros(0, np.uint8))) == 0
    x = vm.encode("e" * 50)
    bound = blk.max_output(len(x))
    out = np.zeros(bound, np.uint8)
    assert L.lrhip_stage_execute(blk.stage_handle(), x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), bound - 1) < 0
    assert "output capacity %d <" % (bound - 1) in _lib.last_error()
    assert L.lrhip_stage_execute(blk.stage_handle(), x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), bound) == 50
    assert text_of(out[:50]) == b"e" * 50
    d_in, d_out = L.lrhip_malloc(256), L.lrhip_malloc(256)
    try:
        _lib.check(L.lrhip_memcpy_h2d(d_in, x.ctypes.data_as(C.c_void_p), x.nbytes), "h2d")
        blk.reset()
        with pytest.raises(lr.LrhipError, match="varicodedecoder: output capacity %d < bound %d" % (bound - 1, bound)):
            blk.process_device(d_in, len(x), d_out, bound - 1)
        assert blk.process_device(d_in, len(x), d_out, bound) == 50
    finally:
        L.lrhip_free(d_in)
        L.lrhip_free(d_out)
    assert not L.lrhip_unary_create(b"varicodedecoder:x=1", 0.0, 0.0, 0, 0)
    assert "takes no parameters" in L.lrhip_strerror().decode(), L.lrhip_strerror().decode()
    slicer = lr.SlicerBlock()
    slicer.differentiate([types.Float32])
    slicer.initialize()
    ch = lr.Chain([slicer, decoder()])
    assert ch.max_output(100) == 36 and ch.get_output_type() is types.Byte
    wave = np.where(vm.encode("via a chain") == 1, 0.5, -0.5).astype(np.float32)
    assert text_of(ch.process(wave)) == b"via a chain"
    with pytest.raises(lr.LrhipError):                   # memory() = -1: no time partitions through it
        ch.start_at(4096)


# ---- the receiver --------------------------------------------------------------------------------------------------------------------
def test_bpsk31_receiver_decodes_to_text():
    """a dbpsk31 loopback: idle zeros, a short message, noise 0.3.  Whole and in two calls the receiver's characters are the literal loop's on
    the bits the receiver without the decoder gives on the same calls, and they contain the message."""
    rate = 1000.0
    message = b"CQ CQ de test 123 pse k"
    bits = np.concatenate([np.zeros(128, np.uint8), vm.encode(message), np.zeros(64, np.uint8)])
    x = ds.dbpsk31(bits, rate, noise=0.3, seed=4)
    for edges in ([0, len(x)], [0, len(x) // 2 + 13, len(x)]):
        rx, rx_bits, lit = lr.bpsk31_receiver(rate, decoder=True), lr.bpsk31_receiver(rate), vm.VaricodeLiteral()
        got, want = [], []
        for a, b in zip(edges[:-1], edges[1:]):
            got.append(rx.process(x[a:b]))
            want.append(lit.process(rx_bits.process(x[a:b])))
            assert got[-1].dtype == np.uint8 and np.array_equal(got[-1], want[-1]), (a, b)
        assert message in text_of(np.concatenate(got))
