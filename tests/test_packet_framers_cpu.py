"""The models of the AX.25 and POCSAG framers (tests/helpers/ax25_model.py, pocsag_model.py) against the reference's golden vectors, the eager
POCSAG contract against the literal loop, the AX.25 hop formulation against the literal loop, the layouts of the two frame types and the two
max_output bounds on adversarial streams.  No GPU."""
import numpy as np
import pytest

from luaradio_amd import types
from tests.helpers import ax25_model as A
from tests.helpers import pocsag_model as P


def bit_by_bit(blk, x):
    out = []
    for k in range(len(x)):
        out += blk.process_frames(x[k:k + 1])
    return out


def cut_frames(blk, x, cuts):
    """[frames of each call]"""
    return [blk.process_frames(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def random_cuts(rng, n, count):
    return [0] + sorted(int(c) for c in rng.integers(0, n + 1, count)) + [n]


# ---- goldens
def test_ax25_literal_model_reproduces_the_goldens_whole_and_bit_by_bit():
    cases = A.golden_cases()
    assert sum(len(want) for _, _, want in cases) == 8
    for desc, x, want in cases:
        frames = A.FramerLiteral().process_frames(x)
        assert A.objects(frames) == want, desc
        assert A.objects(bit_by_bit(A.FramerLiteral(), x)) == want, desc
        rec = A.records(frames)
        assert rec.dtype == A.DTYPE and A.pads_are_zero(rec) and types.AX25FrameType.frames(rec) == want, desc
        assert A.objects(A.hop_frames(x)) == want, desc


@pytest.mark.parametrize("eager", [False, True])
def test_pocsag_models_reproduce_the_goldens_whole_and_bit_by_bit(eager):
    cases = P.golden_cases()
    assert all(len(want) >= 6 for _, _, want in cases)
    for desc, x, want in cases:
        assert P.FramerLiteral(eager).process_frames(x) == want, desc
        assert bit_by_bit(P.FramerLiteral(eager), x) == want, desc
        rec = P.records(want)
        assert rec.dtype == P.DTYPE and P.pads_are_zero(rec) and types.POCSAGFrameType.frames(rec) == want, desc


# ---- the eager contract
def pocsag_stream(rng, seed_messages=7, tail=0):
    bits, sent = P.transmission(P.random_messages(rng, seed_messages))
    return np.concatenate([rng.integers(0, 2, 50).astype(np.uint8), P.preamble(), bits, rng.integers(0, 2, tail).astype(np.uint8)]), sent


def test_pocsag_eager_is_cut_invariant_and_brackets_the_literal_loop():
    rng = np.random.default_rng(11)
    streams = [x for _, x, _ in P.golden_cases()[:2]] + [pocsag_stream(rng, 7, tail)[0] for tail in (0, 31, 544, 700)]
    for x in streams:
        n = len(x)
        eager = P.FramerLiteral(True).process_frames(x)
        for trial in range(4):
            cuts = random_cuts(rng, n, 1 + 5 * trial)
            got = sum(cut_frames(P.FramerLiteral(True), x, cuts), [])
            assert got == eager                                            # cut-invariant
            lit = sum(cut_frames(P.FramerLiteral(False), x, cuts), [])
            assert lit == eager[:len(lit)]                                 # whatever the literal loop emits for a cutting is a prefix
        for extra in (544, 576, 1088):
            more = np.concatenate([x, rng.integers(0, 2, extra).astype(np.uint8)])
            lit = P.FramerLiteral(False).process_frames(more)
            assert lit[:len(eager)] == eager                               # ... and 544 further bits bring the literal loop past it


def test_pocsag_the_lag_the_contract_settles():
    """a stream that ends at a batch's last bit: the literal loop in one call has not processed the batch, the eager one has"""
    _, x, want = P.golden_cases()[0]
    start = next(k for k in range(len(x)) if P.correlation(x[k:k + 32]) >= 28)
    cut = x[:start + P.BATCH]
    assert len(P.FramerLiteral(False).process_frames(cut)) == 0
    eager = P.FramerLiteral(True).process_frames(cut)
    assert len(eager) >= 1 and eager == want[:len(eager)]


# ---- the AX.25 hop formulation
def test_ax25_hop_formulation_equals_the_literal_loop():
    rng = np.random.default_rng(12)
    total = 0
    for trial in range(120):
        x = A.random_stream(rng)
        lit = A.records(A.FramerLiteral().process_frames(x))
        assert A.same_records(A.records(A.hop_frames(x)), lit), trial
        total += len(lit)
        if trial % 10 == 0:                                                # the literal loop is cut-invariant
            cuts = random_cuts(rng, len(x), 9)
            assert A.same_records(A.records(sum(cut_frames(A.FramerLiteral(), x, cuts), [])), lit)
    assert total >= 300


def test_ax25_shared_flags_lengths_and_extraction():
    rng = np.random.default_rng(13)
    a, b = A.random_octets(rng), A.random_octets(rng)
    shared = np.concatenate([A.framed(a, 1, 0), A.framed(b, 1, 1)])
    assert A.objects(A.FramerLiteral().process_frames(shared)) == A.objects([A.frame_of(a)])
    apart = np.concatenate([A.framed(a), A.framed(b)])
    assert A.objects(A.FramerLiteral().process_frames(apart)) == A.objects([A.frame_of(a), A.frame_of(b)])
    # 13 octets are accepted and 12 refused; 396 octets (3184 unstuffed bits) are the most
    assert len(A.FramerLiteral().process_frames(A.framed(A.random_octets(rng, naddr=1, payload_len=4)))) == 1
    assert len(A.FramerLiteral().process_frames(A.framed(A.random_octets(rng, naddr=1, payload_len=4)[:12]))) == 0
    big = A.long_octets(396, 1)
    assert len(A.raw_of(big)) == 3185
    got = A.FramerLiteral().process_frames(A.framed(big))
    assert len(got) == 1 and got[0]["octets"] == big
    assert len(A.raw_of(A.long_octets(396, 2))) == 3186 and len(A.FramerLiteral().process_frames(A.framed(A.long_octets(396, 2)))) == 0
    # the two ways the extraction returns nil
    assert A.frame_of(bytes([0x40] * 20)) is None                          # the address chain runs into the FCS
    assert A.frame_of(bytes([0x40] * 13 + [0x41])) is None                 # the chain ends on the last octet: no control octet
    none = A.frame_of(bytes([0x40] * 13 + [0x41, 0x03]))
    assert none["pid"] is None and none["payload"] is None
    empty = A.frame_of(bytes([0x40] * 13 + [0x41, 0x03, 0xf0]))
    assert empty["pid"] == 0xf0 and empty["payload"] == b""


# ---- the frame types
def test_frame_type_layouts_and_round_trips():
    def layout(t):
        return {k: (v[1], v[0].itemsize, v[0].shape) for k, v in t.dtype.fields.items()}
    assert (types.AX25FrameType.size, types.AX25FrameType.dtype.itemsize) == (416, 416)
    assert layout(types.AX25FrameType) == {"length": (0, 2, ()), "crc": (2, 2, ()), "num_addresses": (4, 1, ()), "control": (5, 1, ()), "pid": (6, 1, ()),
                                           "has_pid": (7, 1, ()), "payload_offset": (8, 2, ()), "payload_length": (10, 2, ()), "data": (16, 400, (400,))}
    assert (types.POCSAGFrameType.size, types.POCSAGFrameType.dtype.itemsize) == (256, 256)
    assert layout(types.POCSAGFrameType) == {"address": (0, 4, ()), "func": (4, 1, ()), "flags": (5, 1, ()), "count": (6, 2, ()), "data": (8, 248, (62,))}
    for t in (types.AX25FrameType, types.POCSAGFrameType):
        assert all(t.dtype[k].base.byteorder in ("<", "=", "|") for k in t.dtype.names)
        assert t.vector(3).shape == (3,) and t.vector(3).dtype == t.dtype and t.frames(t.vector(0)) == []
    rng = np.random.default_rng(14)
    frames = [A.frame_of(A.random_octets(rng, pid=bool(k % 2))) for k in range(6)]
    assert types.AX25FrameType.frames(A.records(frames)) == A.objects(frames)
    assert [f["pid"] is None for f in frames] == [True, False] * 3
    long = [{"address": 5, "func": 1, "data": list(range(n))} for n in (0, 1, 62, 63, 124, 125, 130)]
    rec = P.records(long)
    assert [int(c) for c in rec["count"]] == [0, 1, 62, 62, 1, 62, 62, 62, 62, 1, 62, 62, 6]
    assert [int(f) for f in rec["flags"]] == [0, 0, 0, 1, 2, 1, 2, 1, 3, 2, 1, 3, 2]
    assert types.POCSAGFrameType.frames(rec) == long


# ---- the bounds
def ax25_bound(n):
    return (n + 135) // 136


def pocsag_bound(n):
    return (n + 543) // 32


def test_ax25_max_output_on_minimal_frames_back_to_back():
    rng = np.random.default_rng(15)
    x = np.concatenate([A.framed(A.minimal_octets(seed)) for seed in range(12)])
    assert len(x) == 12 * 136
    assert len(A.FramerLiteral().process_frames(x)) == 12 == ax25_bound(len(x))
    for cuts in ([0, len(x)], list(range(0, len(x) + 1, 136)), list(range(0, len(x) + 1, 8)), list(range(135, len(x), 136)) + [len(x)],
                 [0, 135, 136, 271, 272, len(x)], random_cuts(rng, len(x), 20)):
        cuts = sorted(set([0] + cuts + [len(x)]))
        blk = A.FramerLiteral()
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert len(blk.process_frames(x[a:b])) <= ax25_bound(b - a), (a, b)
    blk = A.FramerLiteral()
    assert sum(len(blk.process_frames(x[k:k + 1])) for k in range(len(x))) == 12         # one bit per call: bound 1, one frame at most


def test_pocsag_max_output_on_adversarial_streams():
    rng = np.random.default_rng(16)
    bad = P.bits_of(P.address_codeword(1, 0) ^ 3)                           # two errors: uncorrectable (the code's distance is 6)
    assert P.correct_codeword(P.tonumber(bad, 0, 32)) is None

    def addresses():
        return P.batch_bits([P.address_codeword(int(rng.integers(0, 1 << 18)), int(rng.integers(0, 4))) for _ in range(16)])
    abort = np.concatenate([P.bits_of(P.SYNC_CODEWORD), bad, bad])         # aborts at j = 2 with the next sync word right behind
    x = np.concatenate([addresses(), addresses(), abort, addresses(), abort, abort, addresses(), np.zeros(544, np.uint8)])
    eager = P.FramerLiteral(True).process_frames(x)
    assert len(eager) == 64 and len(P.records(eager)) == 64
    for cuts in ([0, len(x)], list(range(0, len(x), 32)), list(range(0, len(x), 544)), list(range(543, len(x), 544)), list(range(0, len(x), 545)),
                 random_cuts(rng, len(x), 30), list(range(len(x)))):
        cuts = sorted(set([0] + cuts + [len(x)]))
        blk, got = P.FramerLiteral(True), []
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = blk.process(x[a:b])
            assert len(part) <= pocsag_bound(b - a), (a, b)
            got.append(part)
        assert P.same_records(P.concat(got), P.records(eager))
    # a long message: the chain records count too, each in the call in which its 63rd word arrives
    bits, sent = P.transmission([(77, 2, list(range(200)))])
    x = np.concatenate([bits, np.zeros(544, np.uint8)])
    assert P.FramerLiteral(True).process_frames(x) == sent and len(P.records(sent)) == 4
    blk = P.FramerLiteral(True)
    parts = [blk.process(x[a:a + 32]) for a in range(0, len(x), 32)]
    assert all(len(p) <= 1 for p in parts) and [len(p) for p in parts].index(1) < 100        # the first chain record long before the frame ends
    assert P.same_records(P.concat(parts), P.records(sent))
