"""RDSFramerBlock and rds_receiver on the MI355X.  The framer's records are compared for exact equality with the literal model of rdsframer.lua
(tests/helpers/rds_model.py) - golden vectors, random streams with frames of every kind at the sizes where the kernels take another path, every
frame position against a tile and a call boundary, overlapping valid windows, bytes other than 0 / 1, the bookkeeping - and the receiver decodes
the RDS loopback of tests/helpers/rds_signals.py as the reference topology on the CPU does."""
import ctypes as C
import functools

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import rds_model as M
from tests.helpers import rds_signals as S

pytestmark = pytest.mark.gpu

TILE = 1024                            # window starts per workgroup of the match pass (PS_TILE)


def make(cls, args=(), in_types=(types.Bit,), rate=1187.5):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate(list(in_types))
    blk.initialize()
    return blk


def framer():
    return make(lr.RDSFramerBlock)


def same(got, want):
    return got.dtype == np.uint16 and got.ndim == 2 and got.shape[1] == 4 and np.array_equal(got, want)


def cut_run(blk, x, cuts):
    parts = [blk.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.uint16)


def test_goldens_whole_and_bit_by_bit():
    doc = golden_util.load("rdsframer_spec")
    assert len(doc["vectors"]) == 6
    for v in doc["vectors"]:
        x, want = np.asarray(v["inputs"][0], np.uint8), np.asarray(v["outputs"][0], np.uint16).reshape(-1, 4)
        assert np.array_equal(M.RDSFramerLiteral().process(x), want)
        whole, bitwise = golden_util.run_whole_and_samplewise(framer, x)
        assert same(whole, want), v["desc"]
        assert same(bitwise, want), v["desc"]


@functools.lru_cache(maxsize=None)
def stream_case(n):
    """(bits, the literal model's frames, positions inside frames)"""
    if n < 200:
        bits = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
        inside = [n // 2]
        if n >= M.FRAME_LEN:
            bits[n - M.FRAME_LEN:] = M.encode_frame([0x1234, 0xfedc, n, 0xffff])
    else:
        bits, placed = M.random_stream(n, n)
        inside = [placed[k % len(placed)][0] + o for k, o in ((0, 1), (1, 50), (2, 103), (len(placed) // 2, 26), (len(placed) - 1, 77))]
    want = M.RDSFramerLiteral().process(bits)
    bits.setflags(write=False)
    want.setflags(write=False)
    return bits, want, inside


@pytest.mark.parametrize("n", [1, 103, 104, 105, TILE - 1, TILE, TILE + 1, 1 << 18])
def test_random_streams_whole_and_ragged(n):
    bits, want, inside = stream_case(n)
    assert len(want) == (1 if n >= 104 else 0) if n < 200 else len(want) >= 2
    whole = framer().process(bits)
    assert same(whole, want)
    rng = np.random.default_rng(n + 1)
    for trial in range(3):
        cuts = np.unique(np.concatenate([[0, n], inside, rng.integers(0, n + 1, 4 * (trial + 1))]))
        cuts = cuts[(cuts >= 0) & (cuts <= n)]
        assert same(cut_run(framer(), bits, cuts), want)


def test_frame_at_every_offset_before_a_tile_and_a_call_boundary():
    rng = np.random.default_rng(77)
    f = M.encode_frame([0x3aab, 0x02c9, 0x0608, 0x6469])
    blk = framer()
    for off in range(M.FRAME_LEN):
        # the frame starts `off` bits before the second tile of one call
        x = rng.integers(0, 2, TILE + 300).astype(np.uint8)
        x[TILE - off:TILE - off + M.FRAME_LEN] = f
        want = M.RDSFramerLiteral().process(x)
        assert len(want) >= 1
        blk.reset()
        assert same(blk.process(x), want), off
        # ... and `off` bits before the end of a call
        y = rng.integers(0, 2, 700).astype(np.uint8)
        y[350 - off:350 - off + M.FRAME_LEN] = f
        want = M.RDSFramerLiteral().process(y)
        assert len(want) >= 1
        blk.reset()
        assert same(cut_run(blk, y, [0, 350, 700]), want), off


def test_three_tiles_and_a_frame_that_ends_on_the_last_bit():
    """2 TILE + 1 + 103 bits (103: the most the stage carries): the match pass runs exactly three tiles, an odd count, where the 4-byte list of
    tile summaries needs padding in front of the 64-bit lists of the scratch"""
    n = 2 * TILE + 1 + (M.FRAME_LEN - 1)
    x = np.random.default_rng(333).integers(0, 2, n).astype(np.uint8)
    x[100:100 + M.FRAME_LEN] = M.encode_frame([0x1111, 0x2222, 0x3333, 0x4444])
    x[n - M.FRAME_LEN:] = M.encode_frame([0xaaaa, 0x5555, 0x0f0f, 0xf0f0])
    want = M.RDSFramerLiteral().process(x)
    assert len(want) >= 2
    blk = framer()
    assert same(blk.process(x), want)
    blk.reset()
    assert same(cut_run(blk, x, [0, n - 40, n]), want)


def _break_first(x, d):
    for i in range(min(d, M.BLOCK_LEN)):
        for j in range(i + 1, min(d, M.BLOCK_LEN)):
            if (M.PARITY_ROWS[i] ^ M.PARITY_ROWS[j]) not in M.CORRECT_MATRIX:
                y = x.copy()
                y[i] ^= 1
                y[j] ^= 1
                return y
    raise AssertionError("no such pair")


@pytest.mark.parametrize("d", [13, 103])
def test_overlapping_valid_windows(d):
    x = M.overlap_stream(d)
    first, second = M.check_window(x[:104].tolist()), M.check_window(x[d:d + 104].tolist())
    assert first is not None and second is not None
    for stream, words in ((x, first), (_break_first(x, d), second)):
        want = M.RDSFramerLiteral().process(stream)
        assert np.array_equal(want, np.array([words], np.uint16))
        assert same(framer().process(stream), want)
        assert same(cut_run(framer(), stream, [0, d, 104, len(stream)]), want)
        assert same(cut_run(framer(), stream, list(range(len(stream) + 1))), want)
        # in front of a tile boundary as well
        pad = np.zeros(TILE - 50, np.uint8)
        assert same(framer().process(np.concatenate([pad, stream])), want)


def test_only_a_byte_equal_to_one_is_a_one():
    words = [0x3aab, 0x82c8, 0x4849, 0x2918]
    f = M.encode_frame(words)
    pad = np.zeros(40, np.uint8)
    assert same(framer().process(np.concatenate([pad, f, pad])), np.array([words], np.uint16))
    assert len(framer().process(np.concatenate([pad, np.where(f == 1, 255, f).astype(np.uint8), pad]))) == 0
    assert same(framer().process(np.concatenate([pad, np.where(f == 0, 2, f).astype(np.uint8), pad])), np.array([words], np.uint16))


def test_reset_independent_blocks_and_the_empty_call():
    words = [1, 2, 3, 4]
    f = M.encode_frame(words)
    blk = framer()
    assert len(blk.process(f[:60])) == 0
    assert same(blk.process(f[60:]), np.array([words], np.uint16))          # the first 60 bits were carried
    assert len(blk.process(f[:60])) == 0
    blk.reset()
    assert len(blk.process(np.concatenate([f[60:], np.zeros(120, np.uint8)]))) == 0
    a, b = framer(), framer()
    g = M.encode_frame([5, 6, 7, 8])
    assert len(a.process(f[:50])) == 0 and len(b.process(g[:70])) == 0
    assert same(b.process(g[70:]), np.array([[5, 6, 7, 8]], np.uint16))
    assert same(a.process(f[50:]), np.array([words], np.uint16))
    empty = blk.process(np.zeros(0, np.uint8))
    assert empty.shape == (0, 4) and empty.dtype == np.uint16


def test_bounds_and_refusals():
    blk = framer()
    for n in (0, 1, 104, 105, 1 << 20):
        assert blk.max_output(n) == (n + 103) // 104
    L = _lib.load()
    x = np.zeros(208, np.uint8)
    out = np.zeros((2, 4), np.uint16)
    assert L.lrhip_stage_execute(blk.stage_handle(), x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), 1) < 0
    assert "output capacity 1 <" in _lib.last_error()
    d_in, d_out = L.lrhip_malloc(256), L.lrhip_malloc(256)
    try:
        _lib.check(L.lrhip_memcpy_h2d(d_in, x.ctypes.data_as(C.c_void_p), x.nbytes), "h2d")
        with pytest.raises(lr.LrhipError, match="rdsframer: output capacity 1 < bound 2"):
            blk.process_device(d_in, len(x), d_out, 1)
        assert blk.process_device(d_in, len(x), d_out, 2) == 0
    finally:
        L.lrhip_free(d_in)
        L.lrhip_free(d_out)
    assert not L.lrhip_unary_create(b"rdsframer:x=1", 0.0, 0.0, 0, 0)
    assert "takes no parameters" in _lib.last_error()
    with pytest.raises(lr.LrhipError, match="unbounded memory"):
        lr.Chain([framer()]).halo()


def _bit_chain_blocks():
    return [make(lr.SlicerBlock, (), (types.Float32,)), make(lr.ManchesterDecoderBlock), make(lr.DifferentialDecoderBlock), framer()]


def test_bit_chain_graph_ring_and_push():
    frames = np.random.default_rng(9).integers(0, 1 << 16, (40, 4)).astype(np.uint16)
    levels = S.half_symbols(S.frame_bits(frames))
    n = len(levels)
    ch = lr.Chain(_bit_chain_blocks())
    assert ch.get_output_type() is types.RDSFrameType
    assert same(ch.process(levels), frames)
    ch = lr.Chain(_bit_chain_blocks())
    assert same(np.concatenate([ch.process(levels[a:a + 1777]) for a in range(0, n, 1777)]), frames)
    g = lr.DeviceGraph()
    src = g.input("in", types.Float32, 2375.0)
    g.connect(src, lr.SlicerBlock(), lr.ManchesterDecoderBlock(), lr.DifferentialDecoderBlock(), lr.RDSFramerBlock())
    g.initialize()
    got = [g.process(**{"in": levels[a:a + 2999]})["RDSFramerBlock"] for a in range(0, n, 2999)]
    assert all(p.dtype == np.uint16 and p.shape[1:] == (4,) for p in got)
    assert same(np.concatenate(got), frames)
    ch = lr.Chain(_bit_chain_blocks())
    ch.set_ring(3, 2048)
    assert same(np.concatenate(list(ch.stream(levels[a:a + 2048] for a in range(0, n, 2048)))), frames)
    ch = lr.Chain(_bit_chain_blocks())
    ch.set_ring(3, 2048)
    parts = [ch.push(levels[a:a + 701]) for a in range(0, n, 701)]
    parts.append(ch.flush())
    assert all(p.dtype == np.uint16 and p.shape[1:] == (4,) for p in parts)
    assert same(np.concatenate(parts), frames)


@pytest.mark.parametrize("theta", [0.0, 1.5])
def test_rds_receiver_loopback(theta):
    x, sent = S.rds_signal(theta)
    model = S.reference_frames(theta)
    got = lr.rds_receiver(S.FS, -250e3).process(**{"in": x})
    assert list(got) == ["frames"]
    frames = got["frames"]
    print("theta %.1f: device %d frames, CPU topology %d, sent %d" % (theta, len(frames), len(model), len(sent)))
    assert frames.dtype == np.uint16 and frames.ndim == 2 and frames.shape[1] == 4
    assert S.in_order(frames, sent)
    assert len(frames) >= len(model) - 1
    bits = lr.rds_receiver(S.FS, -250e3, framer=False).process(**{"in": x})
    assert list(bits) == ["bits"] and bits["bits"].dtype == np.uint8
    assert np.array_equal(M.RDSFramerLiteral().process(bits["bits"]), frames)


def test_rds_receiver_in_ragged_chunks():
    """the PLL's contract across cuts is a tolerance, not bit identity: no exact comparison here"""
    x, sent = S.rds_signal(0.0)
    model = S.reference_frames(0.0)
    g = lr.rds_receiver(S.FS, -250e3)
    cuts = [0, 300001, 300001 + 411113, len(x)]
    frames = np.concatenate([g.process(**{"in": x[a:b]})["frames"] for a, b in zip(cuts[:-1], cuts[1:])])
    print("ragged: device %d frames, CPU topology %d" % (len(frames), len(model)))
    assert frames.dtype == np.uint16 and frames.shape[1] == 4
    assert S.in_order(frames, sent)
    assert len(frames) >= len(model) - 1
