"""BinaryPhaseCorrectorBlock on the MI355X against its CPU models (tests/helpers/phasecorr_model.py): golden vectors, the f64 window mean at
size, chunking and time partitions bit for bit, NaN, the ComplexToReal fold, the BPSK31 tail against the reference's diamond, and the three
digital receivers decoding a known payload from synthetic signals (tests/helpers/digital_signals.py)."""
import ctypes as C

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import digital_signals as ds
from tests.helpers import phasecorr_model as pm

pytestmark = pytest.mark.gpu


def make(cls, args, in_types, rate=1000.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate(in_types)
    blk.initialize()
    return blk


def bpc(N, I):
    return make(lr.BinaryPhaseCorrectorBlock, [N, I], [types.ComplexFloat32])


def cnoise(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_golden_binaryphasecorrector():
    doc = golden_util.load("binaryphasecorrector_spec")
    for v in doc["vectors"]:
        x, want = v["inputs"][0], v["outputs"][0]
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: bpc(*v["args"]), x)
        assert golden_util.max_abs_err(whole, want) <= doc["epsilon"]
        assert golden_util.max_abs_err(samplewise, want) <= doc["epsilon"]
        assert same_bits(whole, samplewise)


@pytest.mark.parametrize("N,I", [(4, 1), (50, 32), (3000, 32), (8000, 7)])
def test_window_mean_parity_at_size(N, I):
    """within one float ulp of the rotation of the f64 window-mean model, every output"""
    n = 1 << 22
    x = cnoise(n, N + I)
    x[: n // 8] *= np.complex64(np.exp(0.7j))                  # a stretch of constant phase offset on top of the noise
    got = bpc(N, I).process(x)
    want = pm.correct(x, N, I, "mean_fast")
    assert np.all(np.abs(got.astype(np.complex128) - want) <= 2.5e-7 * np.abs(x.astype(np.complex128)) + 1e-30)


@pytest.mark.parametrize("N,I", [(50, 32), (4, 1), (8000, 7)])
def test_ragged_calls_bit_identical(N, I):
    n = 1 << 17
    x = cnoise(n, 3)
    whole = bpc(N, I).process(x)
    # cuts shorter than I, a run of one-sample calls, calls longer than N I
    edges = [0, 1, 2, 3, 5, I // 2 + 6, I + 7, 2 * I + 9] + list(range(3 * I + 10, 3 * I + 90)) + [3 * I + 100, 3 * I + 100 + N * I + 5, n // 2 + 3, n]
    edges = sorted(set(e for e in edges if 0 <= e <= n))
    blk = bpc(N, I)
    got = np.concatenate([blk.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert same_bits(got, whole)


def test_time_partitions_bit_identical():
    N, I, n = 50, 32, 1 << 17
    x = cnoise(n, 4)
    full = lr.Chain([bpc(N, I)]).process(x)
    for first in (N * I + 13, 50001, 3 * n // 4 + 31):
        ch = lr.Chain([bpc(N, I)])
        assert ch.halo() == N * I
        s = ch.start_at(first)
        assert s <= first - N * I
        got = ch.process(x[s:])
        assert same_bits(got, full[first:])


def test_nan_measured_sticky_unmeasured_local_and_reset():
    N, I, n = 50, 32, 20000
    x = cnoise(n, 5)
    clean = bpc(N, I).process(x)
    blk = bpc(N, I)
    xm = x.copy()
    xm[3 * I] = np.nan                                       # measured
    xm[5 * I + 3] = np.nan                                   # not measured: but already after the first NaN measurement
    y1 = blk.process(xm[:4000])
    y2 = blk.process(xm[4000:])
    y = np.concatenate([y1, y2])
    assert not np.isnan(y[:3 * I]).any() and np.isnan(y[3 * I:]).all()
    assert same_bits(y[:3 * I], clean[:3 * I])
    blk.reset()
    assert same_bits(blk.process(x), clean)
    xu = x.copy()
    xu[7 * I + 5] = np.nan                                   # only this sample
    y = bpc(N, I).process(xu)
    bad = np.isnan(y.real) | np.isnan(y.imag)
    assert np.flatnonzero(bad).tolist() == [7 * I + 5]
    keep = np.arange(n) != 7 * I + 5
    assert same_bits(y[keep], clean[keep])


def test_bad_parameters_refused():
    L = _lib.load()
    for op in ["binaryphasecorrector:num_samples=0", "binaryphasecorrector:num_samples=16777217", "binaryphasecorrector:num_samples=50:sample_interval=0",
               "binaryphasecorrector:num_samples=2.5", "binaryphasecorrector:sample_interval=32", "binaryphasecorrector:num_samples=5:foo=1"]:
        assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 1), op
        assert _lib.last_error()


def _fold_pair(N, I):
    return [bpc(N, I), make(lr.ComplexToRealBlock, [], [types.ComplexFloat32])]


def test_fold_complextoreal_process_ring_push():
    N, I, n = 50, 32, 1 << 20
    x = cnoise(n, 6)
    want = bpc(N, I).process(x).real.copy()                  # ComplexToReal of the stand-alone corrector
    unfused = lr.Chain(_fold_pair(N, I), _lib.CHAIN_NO_FUSION)
    fused = lr.Chain(_fold_pair(N, I))
    edges = [0, 17, 40000, 40001, 300007, n]
    got_u = np.concatenate([unfused.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert unfused.last_launches == 5
    got_f = np.concatenate([fused.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert fused.last_launches == 4                          # measure, carry, window, rotate (+ real part)
    assert same_bits(got_u, want) and same_bits(got_f, want)
    # the ring
    ch = lr.Chain(_fold_pair(N, I))
    ch.set_ring(3, 65536)
    got = list(ch.stream([x[a:a + 65536] for a in range(0, n, 65536)]))
    assert same_bits(np.concatenate(got), want)
    # push / flush
    ch = lr.Chain(_fold_pair(N, I))
    ch.set_ring(4, 50000)
    got = [ch.push(x[a:a + 30001]) for a in range(0, n, 30001)]
    got.append(ch.flush())
    assert same_bits(np.concatenate(got), want)


def test_fold_takes_over_carried_state():
    """a chain built from a corrector that has already run continues its stream"""
    N, I, n = 50, 32, 50000
    x = cnoise(n, 8)
    want = bpc(N, I).process(x).real.copy()
    blocks = _fold_pair(N, I)
    head = blocks[0].process(x[:20011]).real
    rest = lr.Chain(blocks).process(x[20011:])
    assert same_bits(np.concatenate([head, rest]), want)


def test_bpsk31_tail_equals_reference_diamond():
    """[BPC, ComplexToReal, ClockSampler, Slicer, DifferentialDecoder(true)] against the reference topology (bpsk31receiver.lua:34-40):
    ZC on the real part clocks a Sampler of the complex corrected data, then ComplexToReal -> Slicer -> Decoder"""
    rate = 1000.0
    bits = ds.framed(ds.payload(1500, 11), 11)
    x = ds.dbpsk31(bits, rate, noise=0.3, seed=2)
    g = lr.DeviceGraph()
    src = g.input("in", types.ComplexFloat32, rate)
    pc = lr.BinaryPhaseCorrectorBlock(50)
    zc, smp = lr.ZeroCrossingClockRecoveryBlock(31.25), lr.SamplerBlock()
    g.connect(src, pc)
    g.connect(pc, lr.ComplexToRealBlock(), zc)
    g.connect(pc, "out", smp, "data")
    g.connect(zc, "out", smp, "clock")
    g.connect(smp, lr.ComplexToRealBlock(), lr.SlicerBlock(), lr.DifferentialDecoderBlock(True))
    g.initialize()
    tail = lr.CompositeBlock()
    tail.connect(lr.BinaryPhaseCorrectorBlock(50), lr.ComplexToRealBlock(), lr.ClockSamplerBlock(31.25), lr.SlicerBlock(),
                 lr.DifferentialDecoderBlock(True))
    tail.rate = rate
    tail.differentiate([types.ComplexFloat32])
    tail.initialize()
    edges = [0, 1000, 1001, 20000, len(x)]
    got_g = np.concatenate([g.process(**{"in": x[a:b]})["DifferentialDecoderBlock"] for a, b in zip(edges[:-1], edges[1:])])
    got_t = np.concatenate([tail.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert tail.chain.last_launches == 4 + 4                 # the corrector with the real part, the clock sampler with slicer and decoder
    assert len(got_t) > 1500 and np.array_equal(got_t, got_g)


def test_ax25_receiver_decodes_afsk1200():
    bits = ds.payload(2000, 21)
    x = ds.afsk1200_fm(ds.framed(bits, 21))
    rx = lr.ax25_receiver()
    out = np.concatenate([rx.process(x[a:a + 400000]) for a in range(0, len(x), 400000)])
    assert out.dtype == np.uint8 and ds.contains(out, bits)


def test_pocsag_receiver_decodes_2fsk():
    bits = ds.payload(2000, 22)
    x = ds.fsk2_pocsag(ds.framed(bits, 22))
    g = lr.pocsag_receiver()
    out = np.concatenate([g.process(**{"in": x[a:a + 400000]})["SlicerBlock"] for a in range(0, len(x), 400000)])
    assert out.dtype == np.uint8 and ds.contains(out, bits)


def test_bpsk31_receiver_needs_the_corrector():
    """carrier phase 1.2 +- 0.2 rad and noise: with the corrector the payload is recovered; with an identity in its place (the real part is then
    only cos 1.2 = 0.36 of the symbol) it is lost"""
    rate = 1000.0
    bits = ds.payload(2000, 23)
    x = ds.dbpsk31(ds.framed(bits, 23), rate, phase=1.2, drift=0.2, noise=1.0, seed=3)
    rx = lr.bpsk31_receiver(rate)
    out = rx.process(x)
    assert ds.contains(out, bits)
    ident = lr.CompositeBlock()
    ident.connect(lr.LowpassFilterBlock(128, 100), lr.RootRaisedCosineFilterBlock(101, 1, 31.25), lr.MultiplyConstantBlock(1.0),
                  lr.ComplexToRealBlock(), lr.ClockSamplerBlock(31.25), lr.SlicerBlock(), lr.DifferentialDecoderBlock(True))
    ident.rate = rate
    ident.differentiate([types.ComplexFloat32])
    ident.initialize()
    assert not ds.contains(ident.process(x), bits)
