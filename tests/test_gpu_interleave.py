"""InterleaveBlock, DeinterleaveBlock, WAVFileSink and WAVFileSource on the device: the reference's golden vectors through the blocks, the four
stages inside guard words (tests/helpers/guarded.py) at every tile edge and port alignment, the WAV conversions byte for byte against the C
oracle, the port-table refusals, the blocks in a DeviceGraph, the interleaved stereo receiver and a WAV file written and read back.

Everything here is bit-exact: the stages move bytes or apply the conversion of the file sinks and sources, whose oracle is exact."""
import ctypes as C
import io

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from oracle import oracle as O
from tests import golden_util as G
from tests.helpers import guarded as GD
from tests.helpers import interleave_model as M
from tests.test_gpu_bounds import RawStage, TorchMemory

pytestmark = pytest.mark.gpu

NS = [2, 3, 4, 5, 8, 32]


def T(N, words):
    """frames of one workgroup tile: kernels_interleave.h il_tile_frames() = (IL_TILE_WORDS / (N * W)) & ~15, IL_TILE_WORDS = 4096, W = words of
    a planar element (1: Float32 and the WAV forms, 2: ComplexFloat32).  The LDS-transpose form serves every N and every alignment."""
    return (4096 // (N * words)) & ~15


def T2(words):
    """frames of one workgroup of the register-only Interleave of two channels, which runs when all three pointers are 16-byte aligned:
    stage_interleave.h grid_for(nitems + 1, IL_THREADS), nitems = n / (4 / W) - 256 threads of one 16-byte vector per channel"""
    return 256 * 4 // words


def frame_counts(N, words, interleave=False):
    out = {0, 1, N - 1, N, N + 1}
    for t in [T(N, words)] + ([T2(words)] if interleave and N == 2 else []):
        out |= {2 * t + 1, 2 * t + 2, 2 * t + 3, 3 * t - 1, 3 * t}
    return sorted(out)


def stage(op):
    return RawStage(_lib.load().lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0), op)


def offset_patterns(ports):
    """elements between a 16-byte boundary and each port's pointer (the single-ported side is the last entry): all aligned, all off by one, and
    the two alternations - every port meets both alignments next to neighbours of either"""
    return [[0] * ports, [1] * ports, [k % 2 for k in range(ports)], [(k + 1) % 2 for k in range(ports)]]


def run_ports(obj, many_in, ins, n_arg, want, cap, in_elem, out_elem, offs, in_kind="float", out_floats=None, seed=0):
    """one device call of a many-ported stage inside guard words, once with hostile and once with finite bytes around the inputs.
    ins: one array per input port; want: the expected array per output port (its length is the port's count); cap: capacity of each output
    port in elements; offs: elements (of the port's own size) between the 16-byte boundary and each pointer, inputs first."""
    mem, L = TorchMemory(), _lib.load()
    ins = [np.ascontiguousarray(x) for x in ins]
    runs = []
    for hostile in (True, False):
        rng = np.random.default_rng(seed + 977)
        ibufs = [GD.Buffer(mem, offs[p] * in_elem, max(x.nbytes, 0)) for p, x in enumerate(ins)]
        obufs = [GD.Buffer(mem, offs[len(ins) + p] * out_elem, cap * out_elem) for p in range(len(want))]
        images = [GD._input_image(b.size, b.lo, np.frombuffer(x.tobytes(), np.uint8), in_kind, hostile, rng) for b, x in zip(ibufs, ins)]
        for b, img in zip(ibufs, images):
            mem.write(b.h, img)
        for b in obufs:
            mem.write(b.h, GD.sentinel_fill(b.size))
        mem.sync()
        table = _lib.port_table([b.addr() for b in (ibufs if many_in else obufs)])
        at = C.addressof(table)
        try:
            got = L.lrhip_stage_execute_device(obj.stage_handle(), at if many_in else ibufs[0].addr(), n_arg, obufs[0].addr() if many_in else at, cap)
            _lib.check(got, "execute_device")
            mem.sync()
        except (RuntimeError, _lib.LrhipError) as e:
            if any(w in str(e) for w in ("illegal memory access", "launch failure", "hipErrorIllegal")):
                pytest.exit("GPU fault at n = %d, offsets %s: %s - nothing more is started on this device" % (n_arg, offs, e), 3)
            raise
        outs = []
        for p, (b, w) in enumerate(zip(obufs, want)):
            y = mem.read(b.h)
            nbytes = len(w) * out_elem
            GD.check_before(y, b.lo, "out%d" % p)
            GD.check_after(y, b.lo, nbytes, "out%d" % p)
            GD.check_written(y, b.lo, nbytes, out_elem, out_floats, "out%d" % p)
            outs.append(y[b.lo:b.lo + nbytes].copy())
        for p, (b, img) in enumerate(zip(ibufs, images)):
            GD.check_input_untouched(img, mem.read(b.h), b.lo, "in%d" % p)
        runs.append((got, outs))
    GD.check_same([np.concatenate(runs[0][1])], [np.concatenate(runs[1][1])])
    for p, w in enumerate(want):
        assert runs[0][1][p].tobytes() == np.ascontiguousarray(w).tobytes(), "out%d differs from the model" % p
    return runs[0][0]


def rand(rng, n, cplx):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    return (x + 1j * rng.uniform(-1, 1, n).astype(np.float32)).astype(np.complex64) if cplx else x


def where(what, **kw):
    return "%s (%s)" % (what, ", ".join("%s = %s" % i for i in kw.items()))


# ---- golden vectors through the blocks --------------------------------------------------------------------------------------------------
def made(cls, args, in_types):
    blk = cls(*args)
    blk.rate = 2.0
    blk.differentiate(in_types)
    blk.initialize()
    return blk


def test_interleave_golden():
    doc = G.load("interleave_spec")
    for v in doc["vectors"]:
        tp = types.ComplexFloat32 if v["inputs"][0].dtype == np.complex64 else types.Float32
        blk = made(lr.InterleaveBlock, v["args"], [tp] * len(v["inputs"]))
        whole = blk.process(*v["inputs"])
        assert whole.dtype == v["outputs"][0].dtype and np.array_equal(whole, v["outputs"][0]), v["desc"]
        parts = [blk.process(*[x[i:i + 1] for x in v["inputs"]]) for i in range(len(v["inputs"][0]))]
        assert np.array_equal(np.concatenate(parts), v["outputs"][0]), v["desc"]
        assert len(blk.process(*[x[:0] for x in v["inputs"]])) == 0


def test_deinterleave_golden():
    doc = G.load("deinterleave_spec")
    for v in doc["vectors"]:
        x, N = v["inputs"][0], v["args"][0]
        tp = types.ComplexFloat32 if x.dtype == np.complex64 else types.Float32
        blk = made(lr.DeinterleaveBlock, v["args"], [tp])
        whole = blk.process(x)
        assert [len(y) for y in whole] == [len(w) for w in v["outputs"]], v["desc"]
        for y, w in zip(whole, v["outputs"]):
            assert y.dtype == w.dtype and np.array_equal(y, w), v["desc"]
        blk.reset()
        assert blk.index == 0
        got = M.run_cuts(blk.process, x, [1] * len(x), N)
        for y, w in zip(got, v["outputs"]):
            assert np.array_equal(y, w), v["desc"]


def test_wavfilesource_golden():
    doc = G.load("wavfilesource_spec")
    for v in doc["vectors"]:
        data, N, rate = v["args"]
        _, _, bits = lr.parse_wav_header(data[:44])
        want = M.wav_unpack(data[44:], N, bits)                  # bit for bit; the printed vectors to the spec's epsilon
        for frames_per_chunk in (None, 1):                        # the whole file in one chunk, and a frame per chunk
            src = lr.WAVFileSource(data, N)
            src.initialize()
            assert src.get_rate() == rate
            if frames_per_chunk:
                src.chunk_size = N * frames_per_chunk
            got = src.read_all()
            got = (got,) if N == 1 else got
            assert src.process() is None
            for y, w, g in zip(got, want, v["outputs"]):
                assert np.array_equal(y, w), v["desc"]
                assert G.max_abs_err(y, g) <= doc["epsilon"], v["desc"]


# ---- the four stages inside guard words -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("size", [4, 8])
def test_interleave_bounds(size, N):
    cplx, rng = size == 8, np.random.default_rng(N * 10 + size)
    obj = stage("interleave:channels=%d:size=%d" % (N, size))
    counts = frame_counts(N, size // 4, interleave=True)
    xs = [rand(rng, max(counts), cplx) for _ in range(N)]
    for n in counts:
        for offs in offset_patterns(N + 1):
            try:
                ins = [x[:n] for x in xs]
                got = run_ports(obj, True, ins, n, [M.interleave(ins)], max(n * N, 1), size, size, offs, out_floats="<f4")
                assert got == n * N
            except AssertionError as e:
                raise AssertionError(where(str(e), n=n, offsets=offs)) from None


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("size", [4, 8])
def test_deinterleave_bounds(size, N):
    cplx, rng = size == 8, np.random.default_rng(N * 10 + size + 1)
    obj = stage("deinterleave:channels=%d:size=%d" % (N, size))
    lengths = sorted({f * N + r for f in frame_counts(N, size // 4) for r in (0, 1, N - 1)})       # also lengths that are no multiple of N
    x = rand(rng, max(lengths), cplx)
    for n in lengths:
        for offs in offset_patterns(N + 1):
            offs = offs[-1:] + offs[:-1]                          # the input first
            try:
                cap = -(-n // N)
                got = run_ports(obj, False, [x[:n]], n, list(M.deinterleave(x[:n], N)), max(cap, 1), size, size, offs, out_floats="<f4")
                assert got == cap
            except AssertionError as e:
                raise AssertionError(where(str(e), n=n, offsets=offs)) from None


@pytest.mark.parametrize("N", [2, 3, 5])
@pytest.mark.parametrize("cplx", [False, True])
def test_deinterleave_ragged_calls_equal_one_call(cplx, N):
    x = rand(np.random.default_rng(N), 3 * T(N, 2 if cplx else 1) * N + N + 1, cplx)
    tp = types.ComplexFloat32 if cplx else types.Float32
    blk = made(lr.DeinterleaveBlock, [N], [tp])
    whole = blk.process(x)
    want = M.deinterleave(x, N)
    cuts = M.ragged_cuts(300, N, 5) + [len(x) - 301 - N, N - 1, 0, 1, 1]
    blk.reset()
    got = M.run_cuts(blk.process, x, cuts, N)
    for k in range(N):
        assert np.array_equal(whole[k], want[k]) and np.array_equal(got[k], want[k]), (N, k)


WAV_FMT = {8: "u8", 16: "s16le", 32: "s32le"}
EDGES = np.array([1.0, -1.0, 1.0000001, -1.0000001, -0.99999994, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e10], np.float32)


@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_wavpack(bits, N):
    rng = np.random.default_rng(bits + N)
    t = T(N, 1)
    obj = stage("wavpack:channels=%d:bits=%d" % (N, bits))
    # every edge value in every channel position: channel k holds the edge values rotated by k, in front of and behind the random samples
    xs = [np.concatenate([np.roll(EDGES, k), rand(rng, 2 * t + 3, False), np.roll(EDGES, -k)]) for k in range(N)]
    for n in (len(xs[0]), 2 * t + 1, len(EDGES), 1):
        ins = [x[:n] for x in xs]
        want = np.frombuffer(O.format_pack(WAV_FMT[bits], M.interleave(ins)), np.uint8)
        assert len(want) == n * N * bits // 8
        for offs in offset_patterns(N + 1):
            try:
                # the record buffer is guarded in bytes: its offset of one element is one raw sample
                got = run_ports(obj, True, ins, n, [want.view({8: "u1", 16: "<u2", 32: "<u4"}[bits])], n * N, 4, bits // 8, offs)
                assert got == n
            except AssertionError as e:
                raise AssertionError(where(str(e), n=n, offsets=offs)) from None


@pytest.mark.parametrize("bits, fmt", [(8, "u8"), (16, "s16le"), (32, "s32le")])
def test_wavpack_mono_equals_realfilesink(bits, fmt):
    x = np.concatenate([EDGES, rand(np.random.default_rng(bits), 5000, False)])
    fh = io.BytesIO()
    ref = made(lr.RealFileSink, [fh, fmt], [types.Float32])
    ref.process(x)
    out = io.BytesIO()
    snk = made(lr.WAVFileSink, [out, 1, bits], [types.Float32])
    snk.process(x)
    assert out.getvalue()[44:] == fh.getvalue() == O.format_pack(fmt, x)


@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_wavunpack(bits, N):
    rng = np.random.default_rng(100 + bits + N)
    t, rb = T(N, 1), bits // 8
    obj = stage("wavunpack:channels=%d:bits=%d" % (N, bits))
    raw = rng.integers(0, 256, (2 * t + 3) * N * rb, dtype=np.uint8)
    raw[:4 * rb] = np.frombuffer(b"\x00" * rb + b"\xff" * rb + b"\x80" * rb + b"\x7f" * rb, np.uint8)       # the ends of every format's range
    for n in (2 * t + 3, 2 * t + 1, N + 1, 1):
        piece = raw[:n * N * rb]
        flat = O.format_convert(WAV_FMT[bits], piece.tobytes(), False)
        want = [flat[k::N] for k in range(N)]
        for offs in offset_patterns(N + 1):
            offs = offs[-1:] + offs[:-1]
            try:
                got = run_ports(obj, False, [piece.view({8: "u1", 16: "<u2", 32: "<u4"}[bits])], n, want, n, rb, 4, offs, in_kind="raw", out_floats="<f4")
                assert got == n
            except AssertionError as e:
                raise AssertionError(where(str(e), n=n, offsets=offs)) from None


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op, why", [
    ("interleave:channels=33:size=4", "channels must be an integer in 2 .. 32"), ("interleave:channels=1:size=4", "channels must be an integer in 2 .. 32"),
    ("deinterleave:channels=2.5:size=8", "channels must be an integer"), ("deinterleave:channels=2:size=2", "size must be 4 or 8"),
    ("wavpack:channels=0:bits=16", "channels must be an integer in 1 .. 32"), ("wavunpack:channels=2:bits=24", "bits must be 8, 16 or 32"),
    ("interleave:channels=2", "missing parameter \"size\""), ("wavpack:channels=2:size=4", "unknown parameter \"size\""),
])
def test_creation_refusals(op, why):
    lr.init()
    assert not _lib.load().lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    assert why in _lib.last_error(), _lib.last_error()


def test_port_table_refusals():
    L, mem = _lib.load(), TorchMemory()
    obj = stage("interleave:channels=2:size=4")
    a, b, y = (GD.Buffer(mem, 0, 64 * 4) for _ in range(3))
    for buf in (a, b, y):
        mem.write(buf.h, GD.sentinel_fill(buf.size))
    mem.sync()
    good = _lib.port_table([a.addr(), b.addr()])

    def refused(table, what):
        rc = L.lrhip_stage_execute_device(obj.stage_handle(), C.addressof(table), 16, y.addr(), 32)
        assert rc < 0 and what in _lib.last_error(), (rc, _lib.last_error())

    wrong_magic = _lib.port_table([a.addr(), b.addr()])
    wrong_magic.magic ^= 1
    refused(wrong_magic, "is not a port table")
    refused(_lib.port_table([a.addr(), b.addr(), a.addr()]), "has 3 ports, the stage has 2 channels")
    refused(_lib.port_table([a.addr(), None]), "port 1 of the port table is null")
    # the entry points that cannot carry a table
    host = np.zeros(64, np.float32)
    rc = L.lrhip_stage_execute(obj.stage_handle(), host.ctypes.data_as(C.c_void_p), 16, host.ctypes.data_as(C.c_void_p), 32)
    assert rc < 0 and "takes a port table" in _lib.last_error(), _lib.last_error()
    rc = L.lrhip_stage_execute2_device(obj.stage_handle(), a.addr(), b.addr(), 16, y.addr(), 32)
    assert rc < 0 and "interleave is not a two-input stage" in _lib.last_error(), _lib.last_error()
    rc = L.lrhip_stage_execute2(obj.stage_handle(), host.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), 16, host.ctypes.data_as(C.c_void_p), 32)
    assert rc < 0 and "interleave is not a two-input stage" in _lib.last_error(), _lib.last_error()
    for create in (lambda arr: L.lrhip_chain_create(arr, 1), lambda arr: L.lrhip_chain_create_ex(arr, 1, 0)):
        arr = (C.c_void_p * 1)(obj.stage_handle())
        assert not create(arr)
        assert "takes a port table and cannot be part of a chain" in _lib.last_error(), _lib.last_error()
    # an output capacity below N n is refused as well
    rc = L.lrhip_stage_execute_device(obj.stage_handle(), C.addressof(good), 16, y.addr(), 31)
    assert rc < 0 and "output capacity 31 < 32" in _lib.last_error(), _lib.last_error()
    mem.sync()
    for buf in (a, b, y):                                        # nothing was launched: not a byte changed
        assert np.array_equal(mem.read(buf.h), GD.sentinel_fill(buf.size))
    assert L.lrhip_stage_execute_device(obj.stage_handle(), C.addressof(good), 16, y.addr(), 32) == 32      # and the stage still works


# ---- DeviceGraph ------------------------------------------------------------------------------------------------------------------------
def test_graph_interleave_of_unequal_chunks():
    rng = np.random.default_rng(7)
    g = lr.DeviceGraph()
    srcs = [g.input(name, types.Float32, 48e3) for name in "abc"]
    il = lr.InterleaveBlock(3)
    for k, s in enumerate(srcs):
        g.connect(s, "out", il, "in%d" % (k + 1))
    g.initialize()
    lens = [(5, 9, 7), (1000, 0, 501), (13, 1009, 510)]          # every input sums to 1018
    xs = [rand(rng, 1018, False) for _ in range(3)]
    pos, got = [0, 0, 0], []
    for call in lens:
        out = g.process(**{name: xs[k][pos[k]:pos[k] + call[k]] for k, name in enumerate("abc")})
        got.append(out["InterleaveBlock"])
        pos = [p + c for p, c in zip(pos, call)]
    shortest = np.min(np.cumsum(lens, axis=0), axis=1)          # a call emits the frames that every input has reached: 5, 9, 1018
    assert [len(y) for y in got] == [3 * int(d) for d in np.diff(np.concatenate([[0], shortest]))] == [15, 12, 3 * 1009]
    assert np.array_equal(np.concatenate(got), M.interleave(xs))


def test_graph_deinterleave_feeds_three_consumers():
    rng = np.random.default_rng(8)
    g = lr.DeviceGraph()
    src = g.input("in", types.Float32, 48e3)
    de = lr.DeinterleaveBlock(3)
    consumers = [lr.MultiplyConstantBlock(2.0), lr.AbsoluteValueBlock(), lr.AddConstantBlock(1.0)]
    for k, c in enumerate(consumers):
        c.name = "c%d" % k
        g.connect(de, "out%d" % (k + 1), c, "in")
    g.connect(src, de)
    g.initialize()
    x = rand(rng, 1000, False)
    got, a = [[], [], []], 0
    for n in (7, 2, 0, 500, 491):
        out = g.process(**{"in": x[a:a + n]})
        for k in range(3):
            got[k].append(out["c%d" % k])
        a += n
    ch = M.deinterleave(x, 3)
    want = [ch[0] * np.float32(2.0), np.abs(ch[1]), ch[2] + np.float32(1.0)]
    for k in range(3):
        assert np.array_equal(np.concatenate(got[k]), want[k]), k


@pytest.mark.parametrize("cplx", [False, True])
def test_graph_deinterleave_interleave_is_the_identity(cplx):
    g = lr.DeviceGraph()
    src = g.input("in", types.ComplexFloat32 if cplx else types.Float32, 48e3)
    de, il = lr.DeinterleaveBlock(3), lr.InterleaveBlock(3)
    g.connect(src, de)
    for k in range(3):
        g.connect(de, "out%d" % (k + 1), il, "in%d" % (k + 1))
    g.initialize()
    x = rand(np.random.default_rng(9), 4001, cplx)
    got, a = [], 0
    for n in M.ragged_cuts(600, 3, 2) + [3400, 1]:
        got.append(g.process(**{"in": x[a:a + n]})["InterleaveBlock"])
        a += n
    assert a == len(x)
    y = np.concatenate(got)
    assert len(y) == 3999 and np.array_equal(y, x[:3999])       # whole frames come out; the last two samples wait for the third


def test_wbfm_stereo_receiver_interleaved():
    fs, n = 1102500.0, 1 << 16
    t = np.arange(n) / fs
    msg = 0.4 * np.sin(2 * np.pi * 1e3 * t) + 0.1 * np.sin(2 * np.pi * 19e3 * t) + 0.3 * np.sin(2 * np.pi * 3e3 * t) * np.sin(2 * np.pi * 38e3 * t)
    iq = np.exp(1j * (2 * np.pi * 250e3 * t + 2 * np.pi * 75e3 / fs * np.cumsum(msg))).astype(np.complex64)
    plain = lr.wbfm_stereo_receiver(fs, -250e3).process(**{"in": iq})
    both = lr.wbfm_stereo_receiver(fs, -250e3, interleaved=True).process(**{"in": iq})
    assert sorted(plain) == ["left", "right"] and sorted(both) == ["stereo"]
    assert len(plain["left"]) == len(plain["right"]) > 2000
    assert np.array_equal(both["stereo"].view(np.uint32), M.interleave([plain["left"], plain["right"]]).view(np.uint32))


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_wav_file_written_by_a_graph_and_read_back(bits):
    rng = np.random.default_rng(bits)
    g = lr.DeviceGraph()
    a, b = g.input("a", types.Float32, 44100), g.input("b", types.Float32, 44100)
    fh = io.BytesIO()
    snk = lr.WAVFileSink(fh, 2, bits)
    g.connect(a, "out", snk, "in1")
    g.connect(b, "out", snk, "in2")
    g.initialize()
    xa, xb = rand(rng, 9000, False), rand(rng, 9000, False)
    assert g.process(a=xa[:100], b=xb[:4000]) == {}
    assert g.process(a=xa[100:], b=xb[4000:]) == {}
    snk.cleanup()
    records = O.format_pack(WAV_FMT[bits], M.interleave([xa, xb]))
    assert fh.getvalue() == lr.wav_header(44100, 2, bits, 9000) + records
    src = lr.WAVFileSource(fh.getvalue(), 2)
    src.initialize()
    left, right = src.read_all()
    assert src.get_rate() == 44100
    flat = O.format_convert(WAV_FMT[bits], records, False)       # the quantised values
    assert np.array_equal(left, flat[0::2]) and np.array_equal(right, flat[1::2])
    assert G.max_abs_err(left, xa) <= {8: 1e-2, 16: 1e-4, 32: 1e-6}[bits]      # and the reference's sink spec bound on the round trip
