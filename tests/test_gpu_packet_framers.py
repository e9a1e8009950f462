"""AX25FramerBlock, POCSAGFramerBlock, ax25_receiver(framer=True) and pocsag_receiver(framer=True) on the MI355X.  The framers' records are compared
for exact equality (every field; pad bytes and unused tail bytes zero) with the literal models of the reference's process() loops
(tests/helpers/ax25_model.py, pocsag_model.py - for POCSAG the eager one, the device's contract): golden vectors, random streams with planted
frames at the sizes where the kernels take another path, every frame position against a tile and a call boundary, the protocols' edge cases,
bytes other than 0 / 1, the bookkeeping, chains and graphs - and the receivers recover the frames that were sent."""
import ctypes as C
import functools

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import ax25_model as A
from tests.helpers import digital_signals as S
from tests.helpers import pocsag_model as P

pytestmark = pytest.mark.gpu

TILE = 1024                            # positions per workgroup of the match passes (PS_TILE)
NAMES = ["ax25", "pocsag"]
BLOCKS = {"ax25": lr.AX25FramerBlock, "pocsag": lr.POCSAGFramerBlock}
OPS = {"ax25": "ax25framer", "pocsag": "pocsagframer"}
MODELS = {"ax25": A, "pocsag": P}
TYPES = {"ax25": types.AX25FrameType, "pocsag": types.POCSAGFrameType}
BOUNDS = {"ax25": lambda n: (n + 135) // 136, "pocsag": lambda n: (n + 543) // 32}


def make(cls, args=(), in_types=(types.Bit,), rate=1200.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate(list(in_types))
    blk.initialize()
    return blk


def framer(name):
    return make(BLOCKS[name])


def model(name):
    return A.FramerLiteral() if name == "ax25" else P.FramerLiteral(eager=True)


def literal(name, x):
    return model(name).process(x)


def run(blk, x):
    """one process() call: the block's own dtype, pad and tail bytes zero"""
    y = blk.process(np.ascontiguousarray(x, np.uint8))
    M = A if y.dtype == A.DTYPE else P
    assert y.dtype == blk.get_output_type().dtype and y.ndim == 1 and M.pads_are_zero(y)
    return y


def cut_run(name, blk, x, cuts):
    cuts = sorted(set(int(c) for c in cuts))
    return MODELS[name].concat([run(blk, x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])


def check(name, x, want=None, cuts=()):
    """the device equals the model (and `want`, when given) whole and for each cutting; returns the records"""
    M = MODELS[name]
    x = np.ascontiguousarray(x, np.uint8)
    lit = literal(name, x)
    if want is not None:
        assert M.same_records(lit, want)
    got = run(framer(name), x)
    assert M.same_records(got, lit)
    for c in cuts:
        assert M.same_records(cut_run(name, framer(name), x, [0, len(x)] + list(c)), lit), c
    return got


MINIMAL = A.minimal_octets()              # 13 octets, no stuffed bit: 136 bits with its flags


def noise(rng, n):
    return rng.integers(0, 2, n).astype(np.uint8)


# ---- goldens
@pytest.mark.parametrize("name", NAMES)
def test_goldens_whole_and_bit_by_bit(name):
    M = MODELS[name]
    for desc, x, want in M.golden_cases():
        lit = literal(name, x)
        assert TYPES[name].frames(lit) == want, desc
        whole, bitwise = golden_util.run_whole_and_samplewise(lambda: framer(name), x)
        assert M.same_records(whole, lit) and M.pads_are_zero(whole), desc
        assert M.same_records(bitwise, lit), desc
        assert TYPES[name].frames(whole) == want, desc


# ---- random planted streams
def ax25_planted(n, seed):
    rng = np.random.default_rng(seed)
    bits = noise(rng, n)
    at, inside, k = int(rng.integers(0, 40)), [], 0
    while len(inside) < 40:
        piece = [A.framed(A.random_octets(rng)),
                 np.concatenate([A.framed(A.random_octets(rng), 1, 0), A.framed(A.random_octets(rng))]),          # a shared flag
                 A.framed(A.random_octets(rng, payload_len=int(rng.integers(100, 380))), 2, 1),
                 np.concatenate([A.framed(A.random_octets(rng))[:-3], A.framed(A.random_octets(rng))])][k % 4]    # a broken closing flag
        if at + len(piece) > n:
            break
        bits[at:at + len(piece)] = piece
        inside += [at + 3, at + len(piece) // 2, at + len(piece) - 4]
        at += len(piece) + (int(rng.integers(0, 2 * TILE)) if n > 4 * TILE else int(rng.integers(0, 30)))
        k += 1
    return bits, inside


def pocsag_planted(n, seed):
    rng = np.random.default_rng(seed)
    bits = noise(rng, n)
    at, inside, k = int(rng.integers(0, 40)), [], 0
    while len(inside) < 40:
        tx, _ = P.transmission(P.random_messages(rng, int(rng.integers(1, 8)), max_words=[6, 6, 70][k % 3]))
        tx = tx.copy()
        for _ in range(k % 4):                                                # single errors, a double error
            tx[int(rng.integers(0, len(tx)))] ^= 1
        piece = np.concatenate([P.preamble(64), tx])
        if at + len(piece) > n:
            break
        bits[at:at + len(piece)] = piece
        inside += [at + 64 + 5, at + 64 + 31, at + 64 + 543, at + 64 + 544 + 17, at + len(piece) - 1]
        at += len(piece) + (int(rng.integers(0, 2 * TILE)) if k % 2 else 0)
        k += 1
    return bits, inside


SIZES = {"ax25": [1, 7, 8, 135, 136, 137, 1023, 1024, 1025, 1 << 16], "pocsag": [1, 31, 32, 543, 544, 545, 1023, 1024, 1025, 1 << 16]}


@functools.lru_cache(maxsize=None)
def stream_case(name, n):
    """(bits, the model's records, positions inside frames and flags / sync words)"""
    if name == "ax25":
        if n < 300:
            bits = noise(np.random.default_rng(n), n)
            f = A.framed(MINIMAL if n >= 136 else A.random_octets(np.random.default_rng(3)))
            if n >= 136:
                bits[n - 136:] = f
            inside = [n // 2, max(n - 4, 0)]
        else:
            bits, inside = ax25_planted(n, n)
    else:
        if n < 1200:
            bits = noise(np.random.default_rng(n), n)
            tx, _ = P.transmission([(0x12345, 1, [1, 2, 3]), (0x54321 + 2, 2, [])])
            k = min(n, len(tx))
            bits[n - k:] = tx[:k]                                             # ends with as much of a batch as fits: at 544 and 545 exactly one
            inside = [n // 2, max(n - 20, 0)]
        else:
            bits, inside = pocsag_planted(n, n)
    want = literal(name, bits)
    bits.setflags(write=False)
    want.setflags(write=False)
    return bits, want, inside


@pytest.mark.parametrize("name,n", [(name, n) for name in NAMES for n in SIZES[name]])
def test_random_streams_whole_and_ragged(name, n):
    M = MODELS[name]
    bits, want, inside = stream_case(name, n)
    if n >= 1 << 16:
        assert len(want) >= 2
    elif name == "ax25" and n in (136, 137):
        assert len(want) == 1                                                 # a minimal frame with its two flags ends the stream
    elif name == "pocsag" and n in (544, 545):
        assert len(want) >= 1                                                 # eager: the batch that ends the stream is processed
    assert M.same_records(run(framer(name), bits), want)
    rng = np.random.default_rng(n + 1)
    for trial in range(3):
        cuts = np.concatenate([[0, n], [c for c in inside if 0 <= c <= n], rng.integers(0, n + 1, 4 * (trial + 1))])
        assert M.same_records(cut_run(name, framer(name), bits, cuts), want)


# ---- every offset against a tile and a call boundary
@pytest.mark.parametrize("name", NAMES)
def test_frame_at_every_offset_before_a_tile_and_a_call_boundary(name):
    M = MODELS[name]
    rng = np.random.default_rng(77)
    if name == "ax25":
        octets = A.random_octets(rng, naddr=2, payload_len=4)                # 20 octets
        assert len(octets) == 20
        f, want, tail = A.framed(octets), A.records([A.frame_of(octets)]), 300
    else:
        tx, sent = P.transmission([(0x1a2b3 * 8 + 1, 3, [0x12345, 0xabcde]), (0x0f0f0 * 8 + 4, 0, [7])], nbatches=1)
        f, want, tail = tx, P.records(sent), 544 + 300                       # the last frame is released by the failed sync test 544 bits on
        assert len(f) == 544
    L = len(f)
    blk = framer(name)
    x = noise(rng, TILE + L + tail)
    half = L + 250
    y = noise(rng, half + L + tail)
    assert len(literal(name, x)) == 0 and len(literal(name, y)) == 0
    found = 0
    for off in range(L):
        # the frame starts `off` bits before the second tile of one call
        xx = x.copy()
        xx[TILE - off:TILE - off + L] = f
        # (AX.25: a flag of the noise that overlaps the frame's opening flag, 7 bits in front of it, takes it - the model says where)
        expect = literal(name, xx) if name == "ax25" else want
        found += len(expect)
        blk.reset()
        assert M.same_records(run(blk, xx), expect), off
        # ... and `off` bits before the end of the first of two calls
        yy = y.copy()
        yy[half - off:half - off + L] = f
        expect = literal(name, yy) if name == "ax25" else want
        found += len(expect)
        blk.reset()
        assert M.same_records(cut_run(name, blk, yy, [0, half, len(yy)]), expect), off
    assert found >= (2 * L - 4) * len(want)
    # the model agrees at the ends and in the middle (POCSAG: it is the same batch in the same noise throughout)
    for off in (0, L // 2, L - 1):
        xx = x.copy()
        xx[TILE - off:TILE - off + L] = f
        assert M.same_records(literal(name, xx), want)


# ---- three tiles, the last frame ends on the last bit
@pytest.mark.parametrize("name", NAMES)
def test_three_tiles_and_a_frame_that_ends_on_the_last_bit(name):
    """2 TILE + 1 + (the most the stage carries: 3192 bytes for AX.25, 543 for POCSAG) bits: three tiles of positions in the stream itself, the
    last one holding a single position in front of the carried length.  The stages size their lists for a full carry on top, which makes 9 tiles
    for AX.25 - an odd count, where the 4-byte list of tile summaries needs padding in front of the 64-bit lists of the scratch - and 4 for POCSAG."""
    M = MODELS[name]
    rng = np.random.default_rng(333)
    if name == "ax25":
        n = 2 * TILE + 1 + A.RAW_MAXLEN + 1 + 7
        first, last = A.framed(MINIMAL), A.framed(A.random_octets(rng, naddr=2, payload_len=4))
    else:
        n = 2 * TILE + 1 + 543
        first = P.transmission([(0x1a2b3 * 8 + 1, 3, [0x12345, 0xabcde]), (0x0f0f0 * 8 + 4, 0, [7])], nbatches=1)[0]
        last = P.transmission([(0x0c0de * 8 + 2, 1, [1, 2, 3]), (0x15555 * 8 + 5, 2, [])], nbatches=1)[0]
        assert len(first) == len(last) == 544
    x = noise(rng, n)
    x[60:60 + len(first)] = first
    x[n - len(last):] = last
    want = literal(name, x)
    assert len(want) >= 2
    blk = framer(name)
    assert M.same_records(run(blk, x), want)
    blk.reset()
    assert M.same_records(cut_run(name, blk, x, [0, n - len(last) // 2, n]), want)


# ---- AX.25 cases
def ax_cuts(x):
    n = len(x)
    return [[n // 3, 2 * n // 3], list(range(0, n, 7)), list(range(0, n, 61))]


def test_ax25_shared_and_overlapping_flags():
    rng = np.random.default_rng(21)
    a, b, c = (A.random_octets(rng) for _ in range(3))
    ra, rb, rc = (A.records([A.frame_of(o)]) for o in (a, b, c))
    pad = noise(rng, 50)
    # two frames sharing one flag give one frame; with two flags they give two; three sharing give the first and the third
    shared = np.concatenate([pad, A.framed(a, 1, 0), A.framed(b), pad])
    check("ax25", shared, ra, ax_cuts(shared))
    apart = np.concatenate([pad, A.framed(a), A.framed(b), pad])
    check("ax25", apart, A.concat([ra, rb]), ax_cuts(apart))
    three = np.concatenate([pad, A.framed(a, 1, 0), A.framed(b, 1, 0), A.framed(c), pad])
    check("ax25", three, A.concat([ra, rc]), ax_cuts(three))
    # overlapping flags 7 apart: 0111111 0111111 0 reads as a flag at 0 and one at 7; the chain takes the first, then searches from 8
    over = np.concatenate([pad, np.array([0, 1, 1, 1, 1, 1, 1], np.uint8), A.framed(a), pad])
    got = check("ax25", over, None, ax_cuts(over))
    assert len(got) == 0                         # the first flag takes the opening flag's 0: the raw frame then starts with 1111110
    over2 = np.concatenate([pad, A.framed(a, 1, 0), np.array([0, 1, 1, 1, 1, 1, 1], np.uint8), A.FLAG_BITS, A.raw_of(b), A.FLAG_BITS, pad])
    check("ax25", over2, None, ax_cuts(over2))
    # an invalid frame whose closing flag opens the next frame
    bad = A.framed(a, 1, 0)
    bad[30] ^= 1
    inv = np.concatenate([pad, bad, A.framed(b), pad])
    check("ax25", inv, rb, ax_cuts(inv))
    # in front of a tile boundary as well
    for before in (1, 9, 100):
        x = np.concatenate([noise(rng, TILE - before - 8), A.framed(a, 1, 0), A.framed(b, 1, 0), A.framed(c), pad])
        check("ax25", x)


def test_ax25_lengths():
    rng = np.random.default_rng(22)
    pad = noise(rng, 30)
    # raw length 3185 is accepted (396 octets), 3186 is not
    big, toobig = A.long_octets(396, 1), A.long_octets(396, 2)
    assert len(A.raw_of(big)) == 3185 and len(A.raw_of(toobig)) == 3186
    x = np.concatenate([pad, A.framed(big), pad])
    got = check("ax25", x, A.records([A.frame_of(big)]), [[1000, 3000], list(range(0, len(x), 997)), [len(pad) + 8 + 3185 + 7]])
    assert int(got["length"][0]) == 396 and got["data"][0][:396].tobytes() == big
    x = np.concatenate([pad, A.framed(toobig), pad])
    assert len(check("ax25", x, None, [[1000, 3000], [len(pad) + 8 + 3185 + 7, len(pad) + 8 + 3186]])) == 0
    # over-length, then a flag, then a frame: the flag behind the over-long stretch opens it
    a = A.random_octets(rng)
    stretch = np.tile(np.array([0, 1, 0, 0, 1, 1, 0, 1], np.uint8), 450)
    x = np.concatenate([A.FLAG_BITS, stretch, A.framed(a), pad])
    check("ax25", x, A.records([A.frame_of(a)]), [[3000, 3300], list(range(0, len(x), 499)), [8 + 3185, 8 + 3186, 8 + 3193, 8 + 3194]])
    # 13 octets accepted, 12 refused
    x = np.concatenate([pad, A.framed(MINIMAL), pad, A.framed(MINIMAL[:12]), pad])
    check("ax25", x, A.records([A.frame_of(MINIMAL)]), ax_cuts(x))


def test_ax25_ones_runs():
    rng = np.random.default_rng(23)
    pad = np.zeros(20, np.uint8)
    # five ones at the frame start: octet 0x1f first, so the raw frame opens 1 1 1 1 1 (0) - ones_count starts at 0 behind the flag
    o = A.random_octets(rng)
    for first in (0x1f, 0x3e, 0xff, 0x7e):
        octets = bytes([first]) + o[1:]
        x = np.concatenate([pad, A.framed(octets), pad])
        want = A.frame_of(octets)
        check("ax25", x, A.records([want]) if want else None, ax_cuts(x))
    # six or more ones inside a frame: the frame is cut there (a flag when exactly six, kept bits when more): never a frame, and equal to the model
    raw = A.raw_of(A.random_octets(rng))
    for ones in (6, 7, 9):
        y = np.concatenate([pad, A.FLAG_BITS, raw[:60], np.zeros(1, np.uint8), np.ones(ones, np.uint8), np.zeros(1, np.uint8), raw[60:], A.FLAG_BITS, pad])
        check("ax25", y, None, ax_cuts(y))


def test_ax25_extraction():
    pad = np.zeros(20, np.uint8)
    cases = {"chain into the FCS": bytes([0x40] * 20), "control missing": bytes([0x40] * 13 + [0x41]), "no PID": bytes([0x40] * 13 + [0x41, 0x03]),
             "PID, empty payload": bytes([0x40] * 13 + [0x41, 0x03, 0xf0]), "56 addresses": bytes([0x40] * 391 + [0x41, 0x03, 0xf0, 0x55, 0xaa])}
    for desc, octets in cases.items():
        want = A.frame_of(octets)
        assert (want is None) == (desc in ("chain into the FCS", "control missing")), desc
        x = np.concatenate([pad, A.framed(octets), pad])
        got = check("ax25", x, A.records([want] if want else []), ax_cuts(x)[:2])
        assert types.AX25FrameType.frames(got) == A.objects([want] if want else []), desc
    got = run(framer("ax25"), np.concatenate([pad, A.framed(cases["no PID"]), A.framed(cases["PID, empty payload"]), A.framed(cases["56 addresses"])]))
    assert [(int(r["has_pid"]), int(r["pid"]), int(r["payload_offset"]), int(r["payload_length"]), int(r["num_addresses"])) for r in got] == \
        [(0, 0, 15, 0, 2), (1, 0xf0, 16, 0, 2), (1, 0xf0, 394, 2, 56)]
    frames = types.AX25FrameType.frames(got)
    assert frames[0]["pid"] is None and frames[0]["payload"] is None and frames[1]["payload"] == b"" and frames[2]["payload"] == b"\x55\xaa"


# ---- POCSAG cases
def pg_stream(messages, nbatches=None, lead=40, seed=5):
    rng = np.random.default_rng(seed)
    tx, sent = P.transmission(messages, nbatches)
    return np.concatenate([noise(rng, lead), P.preamble(64), tx, np.zeros(600, np.uint8)]), sent, lead + 64


def pg_cuts(x, start):
    n = len(x)
    return [[start + 16, start + 544], [start + 543, start + 545, start + 1087], list(range(0, n, 97)), list(range(0, n, 544))]


MESSAGES = [(0x1a2b3 * 8 + 0, 1, [0x11111, 0x22222, 0x33333]), (0x0c0de * 8 + 3, 2, []), (0x15555 * 8 + 6, 0, [0xfffff] * 5)]


def test_pocsag_sync_word_errors():
    x, sent, start = pg_stream(MESSAGES, nbatches=2)
    check("pocsag", x, P.records(sent), pg_cuts(x, start))
    # two errors in the first sync word pass the correlation and fail the correction: 32 bits dropped; the next sync word is found by the search
    y = x.copy()
    y[start + 3] ^= 1
    y[start + 20] ^= 1
    got = check("pocsag", y, None, pg_cuts(y, start))
    assert 0 < len(got) < len(P.records(sent)) or not P.same_records(got, P.records(sent))
    # ... in the second batch's sync word: the pending frame is emitted there
    y = x.copy()
    y[start + 544 + 3] ^= 1
    y[start + 544 + 20] ^= 1
    check("pocsag", y, None, pg_cuts(y, start))
    # one error in a sync word is corrected; three fail the correlation while in BATCH the test is the correction alone
    for flips in ((7,), (1, 9, 30)):
        y = x.copy()
        for k in flips:
            y[start + 544 + k] ^= 1
        check("pocsag", y, P.records(sent) if len(flips) == 1 else None, pg_cuts(y, start))


def test_pocsag_codeword_errors():
    x, sent, start = pg_stream(MESSAGES, nbatches=2)
    want = P.records(sent)
    first_data = start + 32 + 32                  # message 0: address in slot 0, its first data word in slot 1
    # single errors in the message, check and parity bits of a data word, and in an idle word: corrected
    for k in (first_data + 4, first_data + 25, first_data + 31, start + 32 + 5 * 32 + 9):
        y = x.copy()
        y[k] ^= 1
        check("pocsag", y, want, pg_cuts(y, start)[:2])
    # one uncorrectable codeword ends the frame: the data words behind it are dropped
    y = x.copy()
    y[first_data + 32 + 2] ^= 1
    y[first_data + 32 + 3] ^= 1
    got = check("pocsag", y, None, pg_cuts(y, start))
    f = types.POCSAGFrameType.frames(got)
    assert f[0] == {"address": sent[0]["address"], "func": 1, "data": [0x11111]} and f[1:] == sent[1:]
    # two uncorrectable codewords in a row at j = 2, 9 and 16, with the sync word planted right behind: re-sync inside bits already buffered
    for j in (2, 9, 16):
        y = x.copy()
        for slot in (j - 1, j):
            y[start + 32 * slot + 2] ^= 1
            y[start + 32 * slot + 3] ^= 1
        rest, _ = P.transmission(MESSAGES[1:], nbatches=1)
        y = np.concatenate([y[:start + 32 * (j + 1)], rest, np.zeros(600, np.uint8)])
        got = check("pocsag", y, None, pg_cuts(y, start) + [[start + 32 * (j + 1) - 1, start + 32 * (j + 1) + 31]])
        assert types.POCSAGFrameType.frames(got)[-2:] == sent[1:], j


def test_pocsag_long_frames_and_continuation_flags():
    for words, flags in ((0, [0]), (62, [0]), (63, [1, 2]), (130, [1, 3, 2])):
        data = [(w * 7919 + 1) & 0xfffff for w in range(words)]
        x, sent, start = pg_stream([(0x12345 * 8 + 2, 3, data), (0x0beef * 8 + 5, 1, [9])])
        got = check("pocsag", x, P.records(sent), pg_cuts(x, start) + [list(range(0, len(x), 32))])
        assert [int(v) for v in got["flags"]] == flags + [0] and types.POCSAGFrameType.frames(got) == sent
        assert all(int(a) == sent[0]["address"] and int(f) == 3 for a, f in zip(got["address"][:-1], got["func"][:-1]))


def test_pocsag_sync_pattern_in_a_codeword_slot():
    """the sync word in slot 3 of a batch is read as an address codeword (its top bit is 0)"""
    slots = [P.IDLE_CODEWORD] * 16
    slots[2] = P.SYNC_CODEWORD
    slots[3] = P.data_codeword(0x54321)
    x = np.concatenate([P.preamble(64), P.batch_bits(slots), np.zeros(600, np.uint8)])
    got = check("pocsag", x, None, pg_cuts(x, 64))
    assert types.POCSAGFrameType.frames(got) == [{"address": ((P.SYNC_CODEWORD >> 10) & 0x1ffff8) | 1, "func": (P.SYNC_CODEWORD >> 11) & 3, "data": [0x54321]}]


def test_pocsag_pending_frame_across_calls_and_reset():
    slots = [P.IDLE_CODEWORD] * 14 + [P.address_codeword(0x2aaaa, 2), P.data_codeword(0x13579)]
    batch = P.batch_bits(slots)
    want = P.records([{"address": 0x2aaaa * 8 + 7, "func": 2, "data": [0x13579]}])
    blk = framer("pocsag")
    assert len(run(blk, np.concatenate([P.preamble(64), batch]))) == 0        # the frame is pending at the end of the call
    assert len(run(blk, np.zeros(543, np.uint8))) == 0                       # ... and for 543 further bits
    assert P.same_records(run(blk, np.zeros(1, np.uint8)), want)             # released by the failed sync test of the 544th
    # reset() drops the pending frame and the buffer
    assert len(run(blk, np.concatenate([P.preamble(64), batch, np.zeros(300, np.uint8)]))) == 0
    blk.reset()
    assert len(run(blk, np.zeros(2000, np.uint8))) == 0
    # a pending frame that runs on in the next call's batch
    more = P.batch_bits([P.data_codeword(0x02468)] + [P.IDLE_CODEWORD] * 15)
    assert len(run(blk, np.concatenate([P.preamble(64), batch]))) == 0
    assert P.same_records(run(blk, more), P.records([{"address": 0x2aaaa * 8 + 7, "func": 2, "data": [0x13579, 0x02468]}]))


# ---- bytes other than 0 and 1
def test_ax25_bytes_other_than_0_and_1():
    rng = np.random.default_rng(41)
    octets = A.random_octets(rng, payload_len=20)
    f = A.framed(octets)
    want = A.records([A.frame_of(octets)])
    pad = np.zeros(40, np.uint8)
    x = np.concatenate([pad, f, pad])
    check("ax25", x, want)
    # 255 for every 1 gives no frame
    assert len(check("ax25", np.where(x == 1, 255, x))) == 0
    # 2 for every 0 outside the flags: nothing is unstuffed and the CRC never feeds back on them - the model decides
    twos = x.copy()
    body = slice(len(pad) + 8, len(pad) + len(f) - 8)
    twos[body] = np.where(x[body] == 0, 2, x[body])
    check("ax25", twos, None, ax_cuts(twos)[:1])
    # a 2 behind five ones: kept (not unstuffed), and it resets the ones count
    raw = A.raw_of(bytes([0x40] * 6 + [0x41, 0x03, 0xf0, 0x1f, 0x00, 0x1f, 0x3e, 0x00]))
    stuffed = [k for k in range(5, len(raw)) if raw[k] == 0 and raw[k - 5:k].all()]
    assert stuffed
    y = np.concatenate([pad, A.FLAG_BITS, raw, A.FLAG_BITS, pad])
    assert len(check("ax25", y)) == 1
    y[len(pad) + 8 + stuffed[0]] = 2
    check("ax25", y, None, ax_cuts(y)[:1])
    # a 2 inside the CRC span where a 0 was sent: tonumber still reads 0, but the CRC never feeds back on it, so the frame survives exactly
    # when the register's low bit was 0 there - both outcomes occur
    outcomes = set()
    for k in range(len(pad) + 8, len(pad) + 8 + 60):
        if x[k] == 0 and not x[k - 5:k].all():
            y = x.copy()
            y[k] = 2
            outcomes.add(len(check("ax25", y)))
    assert outcomes == {0, 1}


def test_pocsag_bytes_other_than_0_and_1():
    x, sent, start = pg_stream(MESSAGES, nbatches=2)
    want = P.records(sent)
    # 255 for every 1 gives no frame: the codewords read as 0, and the first sync word fails its correction
    assert len(check("pocsag", np.where(x == 1, 255, x))) == 0
    # a 255 under a +1 tap of the correlation passes it whatever the other 31 bytes are
    rng = np.random.default_rng(42)
    z = noise(rng, 3000)
    assert len(literal("pocsag", z)) == 0
    tx, sent1 = P.transmission(MESSAGES[:1], nbatches=1)
    for at in (100, TILE - 10, TILE + 700):
        y = z.copy()
        y[at + 1] = 255                           # tap 1 of the sync word is +1: S(at) holds, and so does S(at - k) wherever tap 1 + k is +1
        check("pocsag", y, None, [[at + 300], list(range(0, len(y), 211))])
        # ... in front of a real batch whose sync word the search must then find again
        y[at + 40:at + 40 + len(tx)] = tx
        y[at + 40 + len(tx):at + 40 + len(tx) + 600] = 0
        check("pocsag", y, None, [[at + 300], list(range(0, len(y), 211))])
    # a 2 inside a codeword where a 0 was sent reads as 0; where a 1 was sent it is a single error
    y = x.copy()
    zero = next(k for k in range(start + 64, start + 96) if x[k] == 0)
    one = next(k for k in range(start + 96, start + 128) if x[k] == 1)
    y[zero] = 2
    y[one] = 2
    check("pocsag", y, want, pg_cuts(y, start)[:2])
    # ... and inside the sync word a 2 counts 3 in the correlation
    y = x.copy()
    y[start + 544 + 1] = 2
    check("pocsag", y, None, pg_cuts(y, start)[:2])


# ---- bookkeeping
@pytest.mark.parametrize("name", NAMES)
def test_reset_independent_blocks_and_the_empty_call(name):
    M = MODELS[name]
    rng = np.random.default_rng(51)
    if name == "ax25":
        (f, fw), (g, gw) = [(A.framed(o), A.records([A.frame_of(o)])) for o in (A.random_octets(rng), A.random_octets(rng))]
    else:
        def one(address):
            tx, sent = P.transmission([(address, 1, [5, 6])], nbatches=1)
            return np.concatenate([tx, np.zeros(544, np.uint8)]), P.records(sent)
        (f, fw), (g, gw) = one(0x123450), one(0x0abcd3)
    cut = min(len(f), len(g)) * 5 // 8 if name == "ax25" else 300          # inside the frame / inside the batch
    blk = framer(name)
    assert len(run(blk, f[:cut])) == 0
    assert M.same_records(run(blk, f[cut:]), fw)               # the first part was carried
    assert len(run(blk, f[:cut])) == 0
    blk.reset()
    assert len(run(blk, np.concatenate([f[cut:], np.zeros(700, np.uint8)]))) == 0
    a, b = framer(name), framer(name)
    assert len(run(a, f[:cut - 9])) == 0 and len(run(b, g[:cut + 9])) == 0
    assert M.same_records(run(b, g[cut + 9:]), gw)
    assert M.same_records(run(a, f[cut - 9:]), fw)
    empty = run(blk, np.zeros(0, np.uint8))
    assert empty.shape == (0,) and empty.dtype == TYPES[name].dtype


@pytest.mark.parametrize("name", NAMES)
def test_bounds_and_refusals(name):
    dtype = TYPES[name].dtype
    blk = framer(name)
    for n in (0, 1, 135, 136, 137, 543, 544, 545, 1 << 20):
        assert blk.max_output(n) == BOUNDS[name](n)
    L = _lib.load()
    n = 2 * 136 if name == "ax25" else 64
    bound = BOUNDS[name](n)
    x = np.zeros(n, np.uint8)
    out = np.zeros(bound, dtype)
    assert L.lrhip_stage_execute(blk.stage_handle(), x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), bound - 1) < 0
    assert "output capacity %d <" % (bound - 1) in _lib.last_error()
    d_in, d_out = L.lrhip_malloc(n), L.lrhip_malloc(bound * dtype.itemsize)
    try:
        _lib.check(L.lrhip_memcpy_h2d(d_in, x.ctypes.data_as(C.c_void_p), x.nbytes), "h2d")
        with pytest.raises(lr.LrhipError, match="%s: output capacity %d < bound %d" % (OPS[name], bound - 1, bound)):
            blk.process_device(d_in, len(x), d_out, bound - 1)
        assert blk.process_device(d_in, len(x), d_out, bound) == 0
    finally:
        L.lrhip_free(d_in)
        L.lrhip_free(d_out)
    assert not L.lrhip_unary_create((OPS[name] + ":x=1").encode(), 0.0, 0.0, 0, 0)
    assert "takes no parameters" in _lib.last_error()
    with pytest.raises(lr.LrhipError, match="unbounded memory"):
        lr.Chain([framer(name)]).halo()


def test_max_output_is_met_but_not_exceeded():
    """the adversarial streams of tests/test_packet_framers_cpu.py: as many records as the bound allows"""
    x = np.tile(A.framed(MINIMAL), 12)
    got = run(framer("ax25"), x)
    assert len(got) == 12 == BOUNDS["ax25"](len(x)) and A.same_records(got, literal("ax25", x))
    rng = np.random.default_rng(16)
    batches = [P.batch_bits([P.address_codeword(int(rng.integers(0, 1 << 18)), int(rng.integers(0, 4))) for _ in range(16)]) for _ in range(3)]
    x = np.concatenate(batches + [np.zeros(544, np.uint8)])
    blk, lit = framer("pocsag"), P.FramerLiteral(True)
    for a in range(0, len(x), 544):
        got = run(blk, x[a:a + 544])
        assert P.same_records(got, lit.process(x[a:a + 544])) and len(got) <= BOUNDS["pocsag"](544)
    assert len(got) == 1


# ---- chains
def _chain_blocks(name):
    return [make(lr.SlicerBlock, (), (types.Float32,)), framer(name)]


@functools.lru_cache(maxsize=None)
def chain_case(name):
    rng = np.random.default_rng(61)
    if name == "ax25":
        bits = np.concatenate([np.concatenate([noise(rng, int(rng.integers(0, 300))), A.framed(A.random_octets(rng))]) for _ in range(12)])
    else:
        bits = np.concatenate([np.concatenate([noise(rng, int(rng.integers(0, 300))), P.preamble(64), P.transmission(P.random_messages(rng, 4))[0]])
                               for _ in range(4)] + [np.zeros(600, np.uint8)])
    want = literal(name, bits)
    assert len(want) >= 12
    return bits, want


@pytest.mark.parametrize("name", NAMES)
def test_slicer_framer_chain_graph_ring_and_push(name):
    M = MODELS[name]
    dtype = TYPES[name].dtype
    bits, want = chain_case(name)
    levels = np.where(bits > 0, 0.7, -0.7).astype(np.float32)
    n = len(levels)
    ch = lr.Chain(_chain_blocks(name))
    assert ch.get_output_type() is TYPES[name]
    assert M.same_records(ch.process(levels), want)
    ch = lr.Chain(_chain_blocks(name))
    assert M.same_records(M.concat([ch.process(levels[a:a + 1777]) for a in range(0, n, 1777)]), want)
    g = lr.DeviceGraph()
    src = g.input("in", types.Float32, 1200.0)
    g.connect(src, lr.SlicerBlock(), BLOCKS[name]())
    g.initialize()
    got = [g.process(**{"in": levels[a:a + 2999]})[BLOCKS[name].name] for a in range(0, n, 2999)]
    assert all(p.dtype == dtype and p.ndim == 1 for p in got)
    assert M.same_records(M.concat(got), want)
    ch = lr.Chain(_chain_blocks(name))
    ch.set_ring(3, 2048)
    assert M.same_records(M.concat(list(ch.stream(levels[a:a + 2048] for a in range(0, n, 2048)))), want)
    ch = lr.Chain(_chain_blocks(name))
    ch.set_ring(3, 2048)
    parts = [ch.push(levels[a:a + 701]) for a in range(0, n, 701)]
    parts.append(ch.flush())
    assert all(p.dtype == dtype and p.ndim == 1 for p in parts)
    assert M.same_records(M.concat(parts), want)


# ---- receivers
RATE, OFFSET = 1e6, -100e3


@pytest.fixture(scope="module")
def ax25_signal():
    rng = np.random.default_rng(71)
    sent = [A.random_octets(rng, naddr=2, payload_len=12), A.random_octets(rng, naddr=3, payload_len=30)]
    bits = np.concatenate([np.tile(A.FLAG_BITS, 24), A.raw_of(sent[0]), np.tile(A.FLAG_BITS, 6), A.raw_of(sent[1]), np.tile(A.FLAG_BITS, 12)])
    # afsk1200_fm NRZI-encodes: a 0 bit changes the tone, which the chain's DifferentialDecoder(True) undoes
    return S.afsk1200_fm(S.framed(bits, 7, lead=64, trail=64), RATE, OFFSET), A.records([A.frame_of(o) for o in sent])


@pytest.fixture(scope="module")
def pocsag_signal():
    tx, sent = P.transmission([(0x1a2b3 * 8 + 1, 1, [0x12345, 0x6789a, 0xbcdef]), (0x00777 * 8 + 4, 3, []), (0x1ffff * 8 + 2, 2, [0x0f0f0] * 9)], nbatches=2)
    assert len(tx) == 2 * 544
    bits = np.concatenate([P.preamble(576), tx, P.preamble(700)])           # reversals behind it: no sync word, and 544 bits to release the last frame
    return S.fsk2_pocsag(S.framed(bits, 8, lead=64, trail=64), RATE, OFFSET), P.records(sent)


def ragged(x, seed, count=7):
    rng = np.random.default_rng(seed)
    edges = [0] + sorted(int(c) for c in rng.integers(1, len(x), count)) + [len(x)]
    return list(zip(edges[:-1], edges[1:]))


def test_ax25_receiver_with_framer(ax25_signal):
    x, sent = ax25_signal
    bits = lr.ax25_receiver(RATE, OFFSET).process(x)
    assert bits.dtype == np.uint8 and np.array_equal(bits, lr.ax25_receiver(RATE, OFFSET, framer=False).process(x))
    got = lr.ax25_receiver(RATE, OFFSET, framer=True).process(x)
    assert got.dtype == A.DTYPE and A.pads_are_zero(got)
    assert A.same_records(got, literal("ax25", bits))
    assert A.same_records(got, sent)
    rx = lr.ax25_receiver(RATE, OFFSET, framer=True)
    assert A.same_records(A.concat([rx.process(x[a:b]) for a, b in ragged(x, 1)]), sent)


def test_pocsag_receiver_with_framer(pocsag_signal):
    x, sent = pocsag_signal
    out = lr.pocsag_receiver(RATE, OFFSET).process(**{"in": x})
    assert list(out) == ["SlicerBlock"] and out["SlicerBlock"].dtype == np.uint8
    bits = out["SlicerBlock"]
    assert np.array_equal(bits, lr.pocsag_receiver(RATE, OFFSET, framer=False).process(**{"in": x})["SlicerBlock"])
    out = lr.pocsag_receiver(RATE, OFFSET, framer=True).process(**{"in": x})
    assert list(out) == ["frames"]
    got = out["frames"]
    assert got.dtype == P.DTYPE and P.pads_are_zero(got)
    assert P.same_records(got, literal("pocsag", bits))
    assert P.same_records(got, sent)
    rx = lr.pocsag_receiver(RATE, OFFSET, framer=True)
    assert P.same_records(P.concat([rx.process(**{"in": x[a:b]})["frames"] for a, b in ragged(x, 2)]), sent)
