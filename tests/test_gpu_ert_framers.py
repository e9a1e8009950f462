"""SCMFramerBlock, SCMPlusFramerBlock, IDMFramerBlock and ert_receiver(framers=True) on the MI355X.  The framers' records are compared for exact
equality (every field; the pad bytes of what a block returns are zero) with the literal models of the reference's process() loops
(tests/helpers/ert_framer_model.py): golden vectors, random streams with frames of every kind at the sizes where the kernels take another path, every frame position against a tile and a call boundary,
overlapping valid windows, the persistent correction of a rejected window, bytes other than 0 / 1, the bookkeeping, chains and graphs - and the
receiver decodes the fields that were sent."""
import ctypes as C
import functools

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import ert_framer_model as M
from tests.helpers import ert_framer_signals as S
from tests.helpers.ert_signals import ERT_DECIMATION, ERT_RATE

pytestmark = pytest.mark.gpu

TILE = 1024                            # window starts per workgroup of the match pass (PS_TILE)
NAMES = ["scm", "scm+", "idm"]
BLOCKS = {"scm": lr.SCMFramerBlock, "scm+": lr.SCMPlusFramerBlock, "idm": lr.IDMFramerBlock}
OPS = {"scm": "scmframer", "scm+": "scmplusframer", "idm": "idmframer"}


def make(cls, args=(), in_types=(types.Bit,), rate=16384.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate(list(in_types))
    blk.initialize()
    return blk


def framer(name):
    return make(BLOCKS[name])


def same(got, want):
    return M.same_records(got, want)


def run(blk, x):
    """one process() call: the block's own dtype, pad bytes zero"""
    y = blk.process(x)
    assert y.dtype == blk.get_output_type().dtype and y.ndim == 1 and M.pads_are_zero(y)
    return y


def cut_run(blk, x, cuts, dtype):
    return M.concat([run(blk, x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])], dtype)


def literal(name, x):
    return M.FramerLiteral(M.PROTOCOLS[name]).process(x)


@pytest.mark.parametrize("name", NAMES)
def test_goldens_whole_and_bit_by_bit(name):
    for desc, x, want in M.golden_cases(name):
        assert same(literal(name, x), want)
        whole, bitwise = golden_util.run_whole_and_samplewise(lambda: framer(name), x)
        assert same(whole, want), desc
        assert same(bitwise, want), desc


def planted_stream(P, n, seed):
    """random bits with frames planted back to back and apart: clean, one message-bit error, one check-bit error, two errors (rejected).
    Returns (bits, [start of each planted frame])"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    starts, at, k = [], int(rng.integers(0, 40)), 0
    while at + P.L <= n and len(starts) < 24:
        f, _ = M.random_frame(P, rng)
        kind = k % 5
        if kind == 1:
            f[P.cw_off + int(rng.integers(0, P.cw_len - 16))] ^= 1
        elif kind == 2:
            f[P.L - 1 - int(rng.integers(0, 16))] ^= 1
        elif kind == 3:
            a, b = M.uncorrectable_pair(P, 5, 40)
            f[P.cw_off + a] ^= 1
            f[P.cw_off + b] ^= 1
        bits[at:at + P.L] = f
        starts.append(at)
        # kind 4 is followed at once by the next frame, the others by a gap that steps through the tile
        at += P.L + (0 if kind == 4 else int(rng.integers(1, 2 * TILE)) if n > 4 * TILE else int(rng.integers(1, 30)))
        k += 1
    return bits, starts


@functools.lru_cache(maxsize=None)
def stream_case(name, n):
    """(bits, the literal model's frames, positions inside frames)"""
    P = M.PROTOCOLS[name]
    if n < 2 * P.L:
        bits = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
        inside = [n // 2]
        if n >= P.L:
            bits[n - P.L:] = M.random_frame(P, np.random.default_rng(n + 7))[0]
    else:
        bits, starts = planted_stream(P, n, n)
        inside = [starts[k % len(starts)] + o for k, o in ((0, 1), (1, P.L // 2), (2, P.L - 1), (len(starts) // 2, P.pre_bits), (len(starts) - 1, P.L - 20))]
    want = literal(name, bits)
    bits.setflags(write=False)
    want.setflags(write=False)
    return bits, want, inside


def stream_sizes(name):
    L = M.PROTOCOLS[name].L
    return [1, L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, 1 << 18]


@pytest.mark.parametrize("name,n", [(name, n) for name in NAMES for n in stream_sizes(name)])
def test_random_streams_whole_and_ragged(name, n):
    P = M.PROTOCOLS[name]
    bits, want, inside = stream_case(name, n)
    if n < 2 * P.L:
        assert len(want) == (1 if n >= P.L else 0)
    elif n >= 1 << 18:
        assert len(want) >= 2
    else:
        assert len(want) >= 1                  # TILE +- 1 holds one IDM frame
    assert same(run(framer(name), bits), want)
    rng = np.random.default_rng(n + 1)
    for trial in range(3):
        cuts = np.unique(np.concatenate([[0, n], inside, rng.integers(0, n + 1, 4 * (trial + 1))]))
        cuts = cuts[(cuts >= 0) & (cuts <= n)]
        assert same(cut_run(framer(name), bits, cuts, P.dtype), want)


@pytest.mark.parametrize("name", NAMES)
def test_frame_at_every_offset_before_a_tile_and_a_call_boundary(name):
    P = M.PROTOCOLS[name]
    rng = np.random.default_rng(77)
    f, fields = M.random_frame(P, rng)
    want = P.record(fields)
    blk = framer(name)
    x = rng.integers(0, 2, TILE + P.L + 300).astype(np.uint8)
    y = rng.integers(0, 2, 2 * P.L + 500).astype(np.uint8)
    half = P.L + 250
    assert len(literal(name, x)) == 0 and len(literal(name, y)) == 0
    for off in range(P.L):
        # the frame starts `off` bits before the second tile of one call
        xx = x.copy()
        xx[TILE - off:TILE - off + P.L] = f
        blk.reset()
        assert same(run(blk, xx), want), off
        # ... and `off` bits before the end of a call
        yy = y.copy()
        yy[half - off:half - off + P.L] = f
        blk.reset()
        assert same(cut_run(blk, yy, [0, half, len(yy)], P.dtype), want), off
    # the model agrees at the ends and in the middle (it is the same frame in the same noise throughout)
    for off in (0, P.L // 2, P.L - 1):
        xx = x.copy()
        xx[TILE - off:TILE - off + P.L] = f
        assert same(literal(name, xx), want)


@pytest.mark.parametrize("name", NAMES)
def test_three_tiles_and_a_frame_that_ends_on_the_last_bit(name):
    """2 TILE + 1 + (L - 1) bits (L - 1: the most the stage carries): three tiles of window starts in the stream itself, the last one holding
    a single position in front of the carried length.  The stage sizes its lists for a full carry on top, which makes 3 tiles for SCM and
    SCM+ - an odd count, where the 4-byte list of tile summaries needs padding in front of the 64-bit lists of the scratch - and 4 for IDM."""
    P = M.PROTOCOLS[name]
    n = 2 * TILE + 1 + (P.L - 1)
    rng = np.random.default_rng(333)
    x = rng.integers(0, 2, n).astype(np.uint8)
    x[50:50 + P.L] = M.random_frame(P, rng)[0]
    x[n - P.L:] = M.random_frame(P, rng)[0]
    want = literal(name, x)
    assert len(want) >= 2
    blk = framer(name)
    assert same(run(blk, x), want)
    blk.reset()
    assert same(cut_run(blk, x, [0, n - P.L // 2, n], P.dtype), want)


@pytest.mark.parametrize("name", NAMES)
def test_overlapping_valid_windows(name):
    P = M.PROTOCOLS[name]
    rng = np.random.default_rng(21)
    pad = np.zeros(TILE - 50, np.uint8)
    for d in (P.pre_bits + 24, P.L - 1):
        x, first, second = M.overlap_stream(P, d, rng)
        # the first broken by two errors in front of the second
        a, b = M.uncorrectable_pair(P, 0, min(d - P.cw_off, 40))
        y = x.copy()
        y[P.cw_off + a] ^= 1
        y[P.cw_off + b] ^= 1
        for stream, fields in ((x, first), (y, second)):
            want = literal(name, stream)
            assert same(want, P.record(fields))                  # one frame: the second is emitted only when the first is not
            assert same(run(framer(name), stream), want)
            assert same(cut_run(framer(name), stream, [0, d, P.L, len(stream)], P.dtype), want)
            assert same(cut_run(framer(name), stream, list(range(0, len(stream), 7)) + [len(stream)], P.dtype), want)
            # in front of a tile boundary as well
            assert same(run(framer(name), np.concatenate([pad, stream])), want)


@pytest.mark.parametrize("name", ["scm+", "idm"])
def test_persistent_correction_of_a_rejected_window(name):
    P = M.PROTOCOLS[name]
    d = P.pre_bits + 16
    stream, fields, flips = M.persistent_case(P)
    want = P.record(fields)
    assert same(literal(name, stream), want) and len(M.pure_window_walk(P, stream)) == 0
    rng = np.random.default_rng(31)
    lead, tail = rng.integers(0, 2, 333).astype(np.uint8), rng.integers(0, 2, 200).astype(np.uint8)
    x = np.concatenate([lead, stream, tail])
    assert same(literal(name, x), want)
    n, w_end, f_end = len(x), len(lead) + P.L, len(lead) + d + P.L
    # whole, and bit by bit
    whole, bitwise = golden_util.run_whole_and_samplewise(lambda: framer(name), x)
    assert same(whole, want)
    assert same(bitwise, want)
    # cut between the mutating window's end and the frame's end: the pending flip crosses a call
    for cut in (w_end, w_end + 1, f_end - 1):
        assert same(cut_run(framer(name), x, [0, cut, n], P.dtype), want), cut
    # the pair straddles a tile boundary: the mutating window starts in one tile, the frame in the next
    for before in (1, d // 2, d - 1):
        xx = np.concatenate([rng.integers(0, 2, TILE - before).astype(np.uint8), stream, tail])
        assert same(literal(name, xx), want)
        assert same(run(framer(name), xx), want), before
    # the flipped bit inside what becomes the carried tail of a call: the call ends right behind it, before the mutating window is complete ...
    flipped_at = len(lead) + d + P.cw_off + flips[0]
    assert flipped_at + 5 < w_end
    for cut in (flipped_at + 1, flipped_at + 5):
        assert same(cut_run(framer(name), x, [0, cut, n], P.dtype), want), cut
    # ... and with the mutating window complete in the first call and the flip in the carried bytes of two calls
    assert same(cut_run(framer(name), x, [0, w_end + 2, w_end + 9, n], P.dtype), want)
    # a second mutating window chained behind the first
    stream2, fields2, _ = M.persistent_case(P, chain=2)
    want2 = P.record(fields2)
    x2 = np.concatenate([lead, stream2, tail])
    assert same(literal(name, x2), want2) and len(M.pure_window_walk(P, x2)) == 0
    assert same(run(framer(name), x2), want2)
    assert same(cut_run(framer(name), x2, [0, len(lead) + P.L + 3, len(lead) + d + P.L + 3, len(x2)], P.dtype), want2)
    assert same(cut_run(framer(name), x2, list(range(0, len(x2), 61)) + [len(x2)], P.dtype), want2)
    # a frame right behind the repaired one is found from the masks again
    nxt, nxt_fields = M.random_frame(P, rng)
    x3 = np.concatenate([x[:f_end], nxt, tail])
    want3 = P.records([fields, nxt_fields])
    assert same(literal(name, x3), want3)
    assert same(run(framer(name), x3), want3)


@pytest.mark.parametrize("name", NAMES)
def test_only_a_byte_equal_to_one_is_a_one(name):
    P = M.PROTOCOLS[name]
    f, fields = M.random_frame(P, np.random.default_rng(41))
    want = P.record(fields)
    pad = np.zeros(40, np.uint8)
    assert same(run(framer(name), np.concatenate([pad, f, pad])), want)
    assert len(run(framer(name), np.concatenate([pad, np.where(f == 1, 255, f).astype(np.uint8), pad]))) == 0
    # 0s replaced by 2 decode as before - except inside the 32 bits idm_compute_crc reads as byte values (idmframer.lua:144: a 2 there is
    # neither a one nor a zero, the serial CRC fails and the literal model rejects the frame): those stay 0 for IDM
    twos = np.where(f == 0, 2, f).astype(np.uint8)
    if name == "idm":
        all_twos = np.concatenate([pad, twos, pad])
        assert len(literal(name, all_twos)) == 0
        assert same(run(framer(name), all_twos), literal(name, all_twos))
        twos[72:104] = f[72:104]
    x = np.concatenate([pad, twos, pad])
    assert same(literal(name, x), want)
    assert same(run(framer(name), x), want)
    # a single-error frame whose erroneous byte is 3 where a 1 was sent: "corrected" to (~3) & 1 = 0, so accepted with that bit still read as 0
    # (for IDM a bit outside the 32 of the serial CRC, which would fail on it)
    k = P.cw_off + (100 if name == "idm" else 45)
    while f[k] != 1:
        k += 1
    g = f.copy()
    g[k] = 3
    x = np.concatenate([pad, g, pad])
    got = run(framer(name), x)
    assert len(got) == 1 and same(got, literal(name, x)) and not same(got, want)
    g[k] = 0
    assert same(got, P.record(P.fields(bytearray(g.tobytes()))))           # the sent fields, but for that bit


@pytest.mark.parametrize("name", NAMES)
def test_reset_independent_blocks_and_the_empty_call(name):
    P = M.PROTOCOLS[name]
    rng = np.random.default_rng(51)
    (f, ff), (g, gf) = M.random_frame(P, rng), M.random_frame(P, rng)
    cut = P.L * 5 // 8
    blk = framer(name)
    assert len(run(blk, f[:cut])) == 0
    assert same(run(blk, f[cut:]), P.record(ff))              # the first part was carried
    assert len(run(blk, f[:cut])) == 0
    blk.reset()
    assert len(run(blk, np.concatenate([f[cut:], np.zeros(P.L + 20, np.uint8)]))) == 0
    a, b = framer(name), framer(name)
    assert len(run(a, f[:cut - 9])) == 0 and len(run(b, g[:cut + 9])) == 0
    assert same(run(b, g[cut + 9:]), P.record(gf))
    assert same(run(a, f[cut - 9:]), P.record(ff))
    empty = run(blk, np.zeros(0, np.uint8))
    assert empty.shape == (0,) and empty.dtype == P.dtype


@pytest.mark.parametrize("name", NAMES)
def test_bounds_and_refusals(name):
    P = M.PROTOCOLS[name]
    blk = framer(name)
    for n in (0, 1, P.L, P.L + 1, 1 << 20):
        assert blk.max_output(n) == (n + P.L - 1) // P.L
    L = _lib.load()
    x = np.zeros(2 * P.L, np.uint8)
    out = np.zeros(2, P.dtype)
    assert L.lrhip_stage_execute(blk.stage_handle(), x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), 1) < 0
    assert "output capacity 1 <" in _lib.last_error()
    d_in, d_out = L.lrhip_malloc(2 * P.L), L.lrhip_malloc(2 * P.dtype.itemsize)
    try:
        _lib.check(L.lrhip_memcpy_h2d(d_in, x.ctypes.data_as(C.c_void_p), x.nbytes), "h2d")
        with pytest.raises(lr.LrhipError, match="%s: output capacity 1 < bound 2" % OPS[name]):
            blk.process_device(d_in, len(x), d_out, 1)
        assert blk.process_device(d_in, len(x), d_out, 2) == 0
    finally:
        L.lrhip_free(d_in)
        L.lrhip_free(d_out)
    assert not L.lrhip_unary_create((OPS[name] + ":x=1").encode(), 0.0, 0.0, 0, 0)
    assert "takes no parameters" in _lib.last_error()
    with pytest.raises(lr.LrhipError, match="unbounded memory"):
        lr.Chain([framer(name)]).halo()


def _chain_blocks(name):
    return [make(lr.SlicerBlock, (), (types.Float32,)), framer(name)]


@pytest.mark.parametrize("name", NAMES)
def test_slicer_framer_chain_graph_ring_and_push(name):
    P = M.PROTOCOLS[name]
    rng = np.random.default_rng(61)
    frames = [M.random_frame(P, rng) for _ in range(12)]
    bits = np.concatenate([np.concatenate([rng.integers(0, 2, int(rng.integers(0, 300))).astype(np.uint8), f]) for f, _ in frames])
    want = literal(name, bits)
    assert same(want, P.records([w for _, w in frames]))
    levels = np.where(bits > 0, 0.7, -0.7).astype(np.float32)
    n = len(levels)
    ch = lr.Chain(_chain_blocks(name))
    assert ch.get_output_type() is P.sample_type
    assert same(ch.process(levels), want)
    ch = lr.Chain(_chain_blocks(name))
    assert same(np.concatenate([ch.process(levels[a:a + 1777]) for a in range(0, n, 1777)]), want)
    g = lr.DeviceGraph()
    src = g.input("in", types.Float32, 16384.0)
    g.connect(src, lr.SlicerBlock(), BLOCKS[name]())
    g.initialize()
    got = [g.process(**{"in": levels[a:a + 2999]})[BLOCKS[name].name] for a in range(0, n, 2999)]
    assert all(p.dtype == P.dtype and p.ndim == 1 for p in got)
    assert same(np.concatenate(got), want)
    ch = lr.Chain(_chain_blocks(name))
    ch.set_ring(3, 2048)
    assert same(np.concatenate(list(ch.stream(levels[a:a + 2048] for a in range(0, n, 2048)))), want)
    ch = lr.Chain(_chain_blocks(name))
    ch.set_ring(3, 2048)
    parts = [ch.push(levels[a:a + 701]) for a in range(0, n, 701)]
    parts.append(ch.flush())
    assert all(p.dtype == P.dtype and p.ndim == 1 for p in parts)
    assert same(np.concatenate(parts), want)


@pytest.fixture(scope="module")
def receiver_case():
    x, frames = S.encoded_signal(0.05)
    return x, S.sent_records(frames)


def test_ert_receiver_with_framers(receiver_case):
    x, sent = receiver_case
    assert len(sent["scm"]) == 2 and len(sent["scm+"]) == 1 and len(sent["idm"]) == 1
    got = lr.ert_receiver(rate=ERT_RATE, decimation=ERT_DECIMATION, framers=True).process(**{"in": x})
    assert sorted(got) == ["idm", "scm", "scm+"]
    # the default still returns the bit streams, and the literal models read the same frames out of them
    bits = lr.ert_receiver(rate=ERT_RATE, decimation=ERT_DECIMATION).process(**{"in": x})
    assert sorted(bits) == ["idm", "scm", "scm+"]
    assert len(bits["scm+"]) == 256                     # its own frame and bits 16 .. 143 of the IDM frame
    for name in NAMES:
        assert bits[name].dtype == np.uint8
        assert same(got[name], sent[name]), name
        assert same(literal(name, bits[name]), got[name]), name
    with pytest.raises(ValueError, match="Unsupported protocol"):
        lr.ert_receiver(("scm", "r900"), rate=ERT_RATE, framers=True)


def test_ert_receiver_with_framers_in_ragged_chunks(receiver_case):
    x, sent = receiver_case
    rng = np.random.default_rng(6)
    edges = [0] + sorted(int(c) for c in rng.integers(1, len(x), 9)) + [len(x)]
    rx = lr.ert_receiver(rate=ERT_RATE, framers=True)
    parts = [rx.process(**{"in": x[a:b]}) for a, b in zip(edges[:-1], edges[1:])]
    for name in NAMES:
        assert all(p[name].dtype == M.PROTOCOLS[name].dtype for p in parts)
        assert same(np.concatenate([p[name] for p in parts]), sent[name]), name
    one = lr.ert_receiver(("idm",), rate=ERT_RATE, framers=True).process(**{"in": x})
    assert list(one) == ["idm"] and same(one["idm"], sent["idm"])
