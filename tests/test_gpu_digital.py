"""Clock recovery, sampler, slicer and differential decoder on the MI355X, bit for bit against the Python models (tests/helpers/digital_model.py):
the reference's golden vectors, random inputs in ragged chunks, and the fused clocksampler [-> slicer -> decoder] through chains, the ring
and push / flush."""
import ctypes as C

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import digital_model as dm

pytestmark = pytest.mark.gpu

RATE = 2.0


def make(cls, args, in_types, rate=RATE):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate(in_types)
    blk.initialize()
    return blk


def test_golden_zerocrossingclockrecovery():
    for v in golden_util.load("zerocrossingclockrecovery_spec")["vectors"]:
        x, want = v["inputs"][0], v["outputs"][0]
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: make(lr.ZeroCrossingClockRecoveryBlock, v["args"], [types.Float32]), x)
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)


def test_golden_sampler():
    for v in golden_util.load("sampler_spec")["vectors"]:
        data, clock = v["inputs"]
        want = v["outputs"][0]
        mk = lambda: make(lr.SamplerBlock, [], [types.type_of(data), types.Float32])  # noqa: E731
        assert np.array_equal(mk().process(data, clock), want)
        blk = mk()
        parts = [blk.process(data[i:i + 1], clock[i:i + 1]) for i in range(len(data))]
        assert np.array_equal(np.concatenate(parts), want)


def test_golden_slicer():
    for v in golden_util.load("slicer_spec")["vectors"]:
        x, want = v["inputs"][0], np.asarray(v["outputs"][0], np.uint8)
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: make(lr.SlicerBlock, v["args"], [types.Float32]), x)
        assert whole.dtype == np.uint8
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)


def test_golden_differentialdecoder():
    for v in golden_util.load("differentialdecoder_spec")["vectors"]:
        x, want = np.asarray(v["inputs"][0], np.uint8), np.asarray(v["outputs"][0], np.uint8)
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: make(lr.DifferentialDecoderBlock, v["args"], [types.Bit]), x)
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)


def signal(n, P, seed, thr=0.0):
    """baseband-like +-1 symbols of P samples with noise, samples equal to the threshold, NaNs, and a DC run of n/3 samples"""
    rng = np.random.default_rng(seed)
    sym = rng.choice([-1.0, 1.0], size=int(n / P) + 2)
    x = (np.repeat(sym, int(np.ceil(P)))[:n] + 0.3 * rng.standard_normal(n)).astype(np.float32)
    x[rng.integers(0, n, n // 50)] = np.float32(thr)
    x[rng.integers(0, n, n // 500)] = np.nan
    a = n // 3
    x[a:a + n // 3] = np.float32(thr + 0.25)
    return x


def crossings(x, thr=0.0):
    """the samples where the clock recovery's hysteresis flips (initially false)"""
    d = np.where(x.astype(np.float64) > thr, 1, np.where(x.astype(np.float64) < thr, -1, 0))
    idx = np.flatnonzero(d)
    dv = d[idx]
    prev = np.concatenate([[-1], dv[:-1]])
    return idx[dv != prev]


def ragged(n, seed, P, x=None):
    """chunk edges at random, inside a symbol, exactly on a crossing of x (the chunk starts with the crossing sample), and two calls inside
    the DC run"""
    rng = np.random.default_rng(seed)
    cuts = set(rng.integers(1, n, 6).tolist()) | {int(7 * P) + 1, n // 3 + 5, n // 3 + n // 9, n // 2}
    if x is not None:
        c = crossings(x)
        if len(c) > 3:
            cuts |= {int(c[2]), int(c[len(c) // 2])}
    return [0] + sorted(c for c in cuts if 0 < c < n) + [n]


def chunked(fn, x, edges):
    return np.concatenate([fn(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])


@pytest.mark.parametrize("n,baud,thr", [(1 << 16, 0.4444, 0.0), (1 << 16, 2.0 / 7.999999, 0.0), (1 << 16, 2.0 / 1.5, 0.0), (1 << 16, 0.5, 0.25),
                                        (1 << 20, 2.0 / (12500 / 1200), 0.0), (1 << 24, 2.0 / (12500 / 512), 0.0)])
def test_zerocrossingclockrecovery_random(n, baud, thr):
    P = RATE / baud
    x = signal(n, P, n + int(P * 100), thr)
    edges = ragged(n, 1, P, x)
    blk = make(lr.ZeroCrossingClockRecoveryBlock, [baud, thr], [types.Float32])
    got = chunked(blk.process, x, edges)
    model = dm.ZcFast(P, thr) if n > (1 << 16) else dm.ZcLiteral(P, thr)
    want = model.process(x)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,cplx", [(1 << 16, False), (1 << 20, True), (1 << 24, False)])
def test_sampler_random(n, cplx):
    rng = np.random.default_rng(n)
    clock = np.repeat(rng.choice([-1.0, 0.0, 1.0, np.nan], size=n // 3 + 1), 3)[:n].astype(np.float32)
    clock[n // 4:n // 4 + n // 3] = 1.0
    data = rng.standard_normal(n).astype(np.float32)
    if cplx:
        data = (data + 1j * rng.standard_normal(n)).astype(np.complex64)
    edges = ragged(n, 2, 3.0)
    blk = make(lr.SamplerBlock, [], [types.type_of(data), types.Float32])
    got = np.concatenate([blk.process(data[a:b], clock[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert np.array_equal(got, dm.SamplerFast().process(data, clock))


@pytest.mark.parametrize("n", [1 << 16, 1 << 24])
def test_slicer_and_decoder_random(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    x[::97] = 0.125
    edges = ragged(n, 3, 5.0)
    sl = make(lr.SlicerBlock, [0.125], [types.Float32])
    assert np.array_equal(chunked(sl.process, x, edges), dm.slicer(x, 0.125))
    b = rng.integers(0, 256, n).astype(np.uint8)
    for inv in (False, True):
        dd = make(lr.DifferentialDecoderBlock, [inv], [types.Bit])
        assert np.array_equal(chunked(dd.process, b, edges), dm.DiffDecModel(inv).process(b))


def _stages(P, thr, tail):
    L = _lib.load()
    ops = [lr.blocks.digital_op("clocksampler", period=P, threshold=thr)]
    if tail >= 1:
        ops.append(lr.blocks.digital_op("slicer", threshold=0.0))
    if tail >= 2:
        ops.append("differentialdecoder:invert=1")
    return [_lib.check_ptr(L.lrhip_unary_create(o.encode(), 0.0, 0.0, 0, 0), o) for o in ops]


def _chain(stages, flags=0):
    L = _lib.load()
    arr = (C.c_void_p * len(stages))(*stages)
    return _lib.check_ptr(L.lrhip_chain_create_ex(arr, len(stages), flags), "chain")


@pytest.mark.parametrize("tail", [0, 1, 2])
@pytest.mark.parametrize("P", [12500 / 1200, 7.999999, 1.5])
def test_clocksampler_chain_vs_model(P, tail):
    L = _lib.load()
    n = 1 << 20 if P == 12500 / 1200 else 1 << 16
    x = signal(n, P, 11)
    model = dm.ClockSamplerModel(P, 0.0, *( [] if tail == 0 else ([0.0] if tail == 1 else [0.0, True])))
    want = model.process(x)
    out_dt = np.float32 if tail == 0 else np.uint8
    for flags in (0, _lib.CHAIN_EXACT):
        stages = _stages(P, 0.0, tail)
        ch = _chain(stages, flags)
        assert L.lrhip_chain_max_output(ch, 1000) == 501
        got = []
        for a, b in zip(ragged(n, 4, P, x)[:-1], ragged(n, 4, P, x)[1:]):
            xi = np.ascontiguousarray(x[a:b])
            out = np.empty(L.lrhip_chain_max_output(ch, len(xi)), out_dt)
            m = _lib.check(L.lrhip_chain_execute(ch, xi.ctypes.data, len(xi), out.ctypes.data, len(out)), "execute")
            got.append(out[:m])
        assert L.lrhip_chain_last_launches(ch) == 4       # summary, carry, emit, pack
        got = np.concatenate(got)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))      # bits: the data has NaNs
        L.lrhip_chain_destroy(ch)
        for s in stages:
            L.lrhip_stage_destroy(s)


def test_clocksampler_fused_equals_unfused_blocks():
    P = 12500 / 1200
    n = 1 << 18
    x = signal(n, P, 5)
    zc = make(lr.ZeroCrossingClockRecoveryBlock, [RATE / P], [types.Float32])
    smp = make(lr.SamplerBlock, [], [types.Float32, types.Float32])
    sl = make(lr.SlicerBlock, [], [types.Float32])
    dd = make(lr.DifferentialDecoderBlock, [True], [types.Bit])
    edges = ragged(n, 6, P)
    unfused = []
    for a, b in zip(edges[:-1], edges[1:]):
        xi = x[a:b]
        unfused.append(dd.process(sl.process(smp.process(xi, zc.process(xi)))))
    unfused = np.concatenate(unfused)
    L = _lib.load()
    stages = _stages(P, 0.0, 2)
    ch = _chain(stages)
    out = np.empty(L.lrhip_chain_max_output(ch, n), np.uint8)
    m = _lib.check(L.lrhip_chain_execute(ch, x.ctypes.data, n, out.ctypes.data, len(out)), "execute")
    assert np.array_equal(out[:m], unfused)
    assert np.array_equal(unfused, dm.ClockSamplerModel(P, 0.0, 0.0, True).process(x))


def test_clocksampler_ring_and_push():
    L = _lib.load()
    P = 12500 / 512
    n, chunk, depth = 1 << 20, 50000, 4
    x = signal(n, P, 9)
    want = dm.ClockSamplerModel(P, 0.0, 0.0, True).process(x)
    stages = _stages(P, 0.0, 2)
    ch = _chain(stages)
    _lib.check(L.lrhip_chain_set_ring(ch, depth, chunk), "set_ring")
    got, pos, pending = [], 0, 0
    cap = L.lrhip_chain_max_output(ch, chunk) + 64
    while pos < n or pending:
        while pos < n and pending < depth:                  # ring-depth chunks before the first collect
            xi = np.ascontiguousarray(x[pos:pos + chunk])
            _lib.check(L.lrhip_chain_submit(ch, xi.ctypes.data, len(xi)), "submit")
            pos += len(xi)
            pending += 1
        out = np.empty(cap, np.uint8)
        m = _lib.check(L.lrhip_chain_collect(ch, out.ctypes.data, cap), "collect")
        got.append(out[:m])
        pending -= 1
    assert np.array_equal(np.concatenate(got), want)
    # push / flush on a fresh chain
    L.lrhip_chain_destroy(ch)
    for s in stages:
        L.lrhip_stage_destroy(s)
    stages = _stages(P, 0.0, 2)
    ch = _chain(stages)
    _lib.check(L.lrhip_chain_set_ring(ch, depth, chunk), "set_ring")
    got = []
    for a in range(0, n, 30001):
        xi = np.ascontiguousarray(x[a:a + 30001])
        bound = L.lrhip_chain_push_bound(ch, len(xi))
        out = np.empty(bound, np.uint8)
        m = _lib.check(L.lrhip_chain_push(ch, xi.ctypes.data, len(xi), out.ctypes.data, bound), "push")
        got.append(out[:m])
    bound = L.lrhip_chain_push_bound(ch, 0)
    out = np.empty(bound, np.uint8)
    m = _lib.check(L.lrhip_chain_flush(ch, out.ctypes.data, bound), "flush")
    got.append(out[:m])
    assert np.array_equal(np.concatenate(got), want)
    L.lrhip_chain_destroy(ch)
    for s in stages:
        L.lrhip_stage_destroy(s)


@pytest.mark.parametrize("P", [12500 / 400, 1.5, 12500 / 1200])
def test_crossing_free_run_many_calls(P):
    """zeros at threshold 0 are never decisive: one crossing-free stretch across 40 calls.  Without the closed form the literal offset is carried
    from call to call, so each call costs its own length; every output equals the literal loop."""
    n, calls = 1 << 15, 40
    rng = np.random.default_rng(3)
    x = np.zeros(n * calls, np.float32)
    x[:2000] = rng.standard_normal(2000).astype(np.float32)
    x[-3000:] = rng.standard_normal(3000).astype(np.float32)
    zc = make(lr.ZeroCrossingClockRecoveryBlock, [RATE / P], [types.Float32])
    cs = make(lr.ClockSamplerBlock, [RATE / P], [types.Float32])
    got_zc = np.concatenate([zc.process(x[k * n:(k + 1) * n]) for k in range(calls)])
    got_cs = np.concatenate([cs.process(x[k * n:(k + 1) * n]) for k in range(calls)])
    assert np.array_equal(got_zc, dm.ZcLiteral(P).process(x))
    assert np.array_equal(got_cs, dm.ClockSamplerModel(P).process(x))


def test_op_string_parameter_is_exact_double():
    """slicer:threshold=%.17g of a double one ulp below a Float32: that Float32 is above it - a threshold parsed through Float32 would say no"""
    f = np.float32(0.1)
    v = float(np.nextafter(np.float64(f), -np.inf))
    assert np.float32(v) == f
    L = _lib.load()
    st = _lib.check_ptr(L.lrhip_unary_create(("slicer:threshold=%.17g" % v).encode(), 0.0, 0.0, 0, 0), "slicer")
    x = np.array([f, np.nextafter(f, np.float32(-1)), np.nextafter(f, np.float32(1))], np.float32)
    out = np.empty(3, np.uint8)
    assert _lib.check(L.lrhip_stage_execute(st, x.ctypes.data, 3, out.ctypes.data, 3), "slicer") == 3
    assert out.tolist() == [1, 0, 1]
    L.lrhip_stage_destroy(st)


@pytest.mark.parametrize("cls,op", [(lr.MultiplyBlock, np.multiply), (lr.AddBlock, np.add), (lr.SubtractBlock, np.subtract)])
def test_binary_blocks_long_calls(cls, op):
    """calls long enough for the host path's pieces (>= 2^20 samples): every piece reads the second input at its own samples"""
    n = (1 << 21) + 3
    rng = np.random.default_rng(4)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    b = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    blk = make(cls, [], [types.ComplexFloat32, types.ComplexFloat32])
    got = blk.process(a, b)
    want = op(a, b) if op is not np.multiply else None
    if want is None:
        ar, ai, br, bi = a.real, a.imag, b.real, b.imag
        want = (ar * br - ai * bi) + 1j * (ar * bi + ai * br)
    assert np.max(np.abs(got - want.astype(np.complex64))) < 1e-5


def test_sampler_in_device_graph_one_sample_calls():
    data = np.random.default_rng(5).standard_normal(64).astype(np.float32)
    clock = np.tile(np.array([-1, 1, 0, 1, -1, -1, 1, 1], np.float32), 8)
    g = lr.DeviceGraph()
    i1, i2 = g.input("d", types.Float32, 2.0), g.input("c", types.Float32, 2.0)
    smp = lr.SamplerBlock()
    g.connect(i1, "out", smp, "data")
    g.connect(i2, "out", smp, "clock")
    g.initialize()
    parts = [next(iter(g.process(d=data[i:i + 1], c=clock[i:i + 1]).values())) for i in range(64)]
    assert np.array_equal(np.concatenate(parts), dm.SamplerModel().process(data, clock))
