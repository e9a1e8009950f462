"""ArbitraryResamplerBlock on the MI355X (luaradio_amd/csrc/kernels_arbresample.h): every output against the f64 model of
tests/helpers/arbresample_model.py inside a bound derived from the arithmetic, the same bits however the stream is cut, after reset() and after seek()
(also 2^40 samples into a stream: the 128-bit positions on the device), both store paths inside guard words, the block inside a Chain, and what the
stage answers through the C ABI."""
import math

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, timeshard, types
from tests.helpers import arbresample_model as am
from tests.helpers import guarded as GD

pytestmark = pytest.mark.gpu

RATE = 44100.0
TILE = 512           # kernels_arbresample.h ARB_TILE: outputs per workgroup tile
# name -> (ratio, options).  At 1 / 16 the 16 taps per phase stretch to T = 256, and 32 phases are the most that fit P * T <= 8192
CASES = {"48000/44100": (48000 / 44100, None), "0.37": (0.37, None), "1/16": (1 / 16, {"phases": 32}), "16": (16.0, None), "1.0": (1.0, None),
         "sqrt(2)": (math.sqrt(2), None), "1+35e-6": (1 + 35e-6, None), "1.3 P=16 T0=4": (1.3, {"phases": 16, "taps_per_phase": 4}),
         "1.3 P=256 T0=32": (1.3, {"phases": 256, "taps_per_phase": 32})}


def tp(cplx):
    return types.ComplexFloat32 if cplx else types.Float32


def make(cls, args, in_type, **attrs):
    blk = cls(*args)
    blk.rate = RATE
    for k, v in attrs.items():
        setattr(blk, k, v)
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def resampler(case, cplx):
    ratio, options = CASES[case]
    return make(lr.ArbitraryResamplerBlock, [ratio, options], tp(cplx))


def rand(seed, n, cplx):
    rng = np.random.default_rng(seed)
    if cplx:
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    return rng.uniform(-1, 1, n).astype(np.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def components(a):
    a = np.asarray(a)
    return np.stack([a.real, a.imag], axis=-1).astype(np.float64) if a.dtype.kind == "c" else a.astype(np.float64)[..., None]


def check_against_model(blk, got, x, m0=0, x0=0, tag=""):
    """every output component within (T + 3) * 2^-24 * sum_k |c_k| * max |x| of the f64 model: one rounding of c_k (<= 2^-24 |c_k|, relative to a
    product with |x| <= max |x|), one rounding per fmaf of the chain of T (each <= 2^-24 of a partial sum, itself <= sum |c_k| max |x|), plus margin"""
    G, D = am.tables_from_taps(blk.taps, blk.phases)
    T = G.shape[1]
    want, sumabs = am.model_f64(x, G, D, blk.step, m0=m0, count=len(got), x0=x0)
    xmax = float(np.max(np.abs(components(x)))) if len(x) else 0.0
    bound = (T + 3) * 2.0 ** -24 * sumabs * xmax
    err = np.max(np.abs(components(got) - components(want)), axis=-1)
    worst = float(np.max(err / bound)) if len(got) else 0.0
    print("%s T = %-3d outputs %-6d max error / bound = %.3f" % (tag, T, len(got), worst))
    assert np.all(err <= bound), (tag, int(np.argmax(err / bound)), worst)


# ---- against the model ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [True, False], ids=["cf32", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_model(case, cplx):
    blk = resampler(case, cplx)
    n = 600 if CASES[case][0] == 16.0 else 6000
    x = rand(11, n, cplx)
    got = blk.process(x)
    assert got.dtype == x.dtype and len(got) == am.output_count(n, blk.step)
    check_against_model(blk, got, x, tag="%s %s" % (case, "cf32" if cplx else "f32"))


# ---- cut invariance, reset, seek ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [True, False], ids=["cf32", "f32"])
@pytest.mark.parametrize("case", ["48000/44100", "0.37", "16"])
def test_any_cut_of_the_stream_gives_the_same_bits(case, cplx):
    n = 300000
    x = rand(12, n, cplx)
    blk = resampler(case, cplx)
    whole = blk.process(x)
    assert len(whole) == am.output_count(n, blk.step)
    blk.reset()
    chunks = [1, 77, 0, 4096, 100000]
    chunks.append(n - sum(chunks))
    parts, pos = [], 0
    for c in chunks:
        parts.append(blk.process(x[pos:pos + c]))
        pos += c
        assert len(parts[-1]) == am.output_count(pos, blk.step) - am.output_count(pos - c, blk.step)
    assert same_bits(np.concatenate(parts), whole)
    # reset() gives the first run's bits again
    blk.reset()
    assert same_bits(blk.process(x[:5000]), whole[:am.output_count(5000, blk.step)])


@pytest.mark.parametrize("cplx", [True, False], ids=["cf32", "f32"])
def test_single_sample_calls_when_decimating_by_16(cplx):
    """fifteen of sixteen calls of one sample return nothing, without error, and carry their sample to the next call"""
    x = rand(13, 9000, cplx)
    blk = resampler("1/16", cplx)
    whole = blk.process(x)
    blk.reset()
    parts = [blk.process(x[j:j + 1]) for j in range(40)]
    assert [len(p) for p in parts] == [1 if j % 16 == 0 else 0 for j in range(40)]
    parts.append(blk.process(x[40:]))
    assert same_bits(np.concatenate(parts), whole)


@pytest.mark.parametrize("cplx", [True, False], ids=["cf32", "f32"])
@pytest.mark.parametrize("case", ["48000/44100", "0.37", "16"])
def test_seek_and_replayed_halo(case, cplx):
    """a partition that owns the stream from n0 on seeks to n0 - (T - 1), replays those T - 1 samples as its halo and drops their outputs: what follows is
    the tail of the uninterrupted run from output ceil(n0 2^48 / step) on, bit for bit"""
    n, n0 = 20000, 12345
    x = rand(14, n, cplx)
    blk = resampler(case, cplx)
    whole = blk.process(x)
    halo = blk.num_taps - 1
    blk.seek(n0 - halo)
    replay = blk.process(x[n0 - halo:n0])
    assert len(replay) == am.output_count(n0, blk.step) - am.output_count(n0 - halo, blk.step)
    tail = blk.process(x[n0:])
    assert same_bits(tail, whole[am.output_count(n0, blk.step):])


@pytest.mark.parametrize("cplx", [True, False], ids=["cf32", "f32"])
@pytest.mark.parametrize("case", ["48000/44100", "0.37", "16"])
def test_seek_far_into_the_stream(case, cplx):
    """2^40 + 3 samples in, m * step needs 128 bits: a stream of zeros with one impulse gives the model's outputs at the model's indices"""
    n0, n = (1 << 40) + 3, 400
    x = np.zeros(n, np.complex64 if cplx else np.float32)
    x[100] = 0.75 - 0.5j if cplx else 0.75
    blk = resampler(case, cplx)
    blk.seek(n0)
    got = blk.process(x)
    m0 = am.output_count(n0, blk.step)
    assert len(got) == am.output_count(n0 + n, blk.step) - m0
    check_against_model(blk, got, x, m0=m0, x0=n0, tag="%s seek 2^40 + 3" % case)
    # the impulse response sits where the model has it, and only there
    G, D = am.tables_from_taps(blk.taps, blk.phases)
    want, _ = am.model_f64(x, G, D, blk.step, m0=m0, count=len(got), x0=n0)
    assert np.array_equal(got == 0, want == 0) and np.count_nonzero(got) > 0


# ---- both store paths inside guard words --------------------------------------------------------------------------------------------------------------
class TorchMemory:
    """device allocations through torch; an address is data_ptr() + byte offset"""

    def __init__(self):
        import torch
        self.torch = torch

    def alloc(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda")

    def write(self, h, data):
        h.copy_(self.torch.from_numpy(np.ascontiguousarray(data)))

    def read(self, h):
        return h.cpu().numpy()

    def addr(self, h, off):
        return h.data_ptr() + off

    def sync(self):
        self.torch.cuda.synchronize()
        _lib.check(_lib.load().lrhip_synchronize(), "synchronize")


def device_call(obj, ins, n, outs, cap):
    return obj.process_device(ins[0], n, outs[0], cap)


@pytest.mark.parametrize("cplx", [True, False], ids=["cf32", "f32"])
@pytest.mark.parametrize("case", ["48000/44100", "0.37", "1/16", "16"])
def test_bounds(case, cplx):
    """consecutive calls of 1, T - 1 and one tile + 1 samples (outputs, when decimating: (TILE + 1) / ratio inputs) into [guard | offset | payload | guard],
    the pointers 16-byte aligned and 4 bytes off: nothing outside the count is written, every output is, the guards' contents do not matter, and the
    values are those of one uncut host call whatever the store path"""
    blk = resampler(case, cplx)
    T, ratio = blk.num_taps, CASES[case][0]
    lens = [1, T - 1, int(math.ceil((TILE + 1) / min(1.0, ratio))), 3]
    x = rand(15, sum(lens), cplx)
    whole = blk.process(x)
    ends = np.cumsum(lens).tolist()
    cuts = [0] + [am.output_count(q, blk.step) for q in ends]
    assert cuts[-1] == len(whole) and cuts[3] - cuts[2] > TILE

    def factory():
        blk.reset()
        return blk

    def check(c, got):
        assert same_bits(got, whole[cuts[c]:cuts[c + 1]]), (c, len(got), cuts[c + 1] - cuts[c])

    mem = TorchMemory()
    for in_off in (0, 4):
        for out_off in (0, 4):
            try:
                GD.run_guarded(factory, [x], lens, in_off, out_off, mem=mem, call=device_call, max_output=lambda obj, n: obj.max_output(n),
                               out_dtype=x.dtype, check=check, offsets_in_bytes=True)
            except (RuntimeError, _lib.LrhipError) as e:
                if any(w in str(e) for w in ("illegal memory access", "launch failure", "hipErrorIllegal")):
                    pytest.exit("GPU fault at offsets %s / %s: %s - nothing more is started on this device" % (in_off, out_off, e), 3)
                raise


def test_capacity_and_null_output_are_refused():
    import torch
    blk = resampler("48000/44100", True)
    n = 1000
    count = am.output_count(n, blk.step)
    x = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    y = torch.zeros(2 * blk.max_output(n), dtype=torch.float32, device="cuda")
    L = _lib.load()
    assert L.lrhip_stage_execute_device(blk.stage_handle(), x.data_ptr(), n, y.data_ptr(), count - 1) < 0
    assert _lib.last_error() == "arbresampler: output capacity %d < %d" % (count - 1, count)
    assert L.lrhip_stage_execute_device(blk.stage_handle(), x.data_ptr(), n, None, count) < 0
    assert "null" in _lib.last_error()
    # nothing was consumed: the counters did not move
    assert blk.process_device(x.data_ptr(), n, y.data_ptr(), count) == count


# ---- in a Chain ------------------------------------------------------------------------------------------------------------------------------------------
def chain_blocks():
    return [make(lr.LowpassFilterBlock, [64, 0.4, 1.0], types.ComplexFloat32, use_fft=lr.block.fir_mode(False)),
            make(lr.ArbitraryResamplerBlock, [48000 / 44100], types.ComplexFloat32), make(lr.ComplexMagnitudeBlock, [], types.ComplexFloat32)]


def test_in_a_chain():
    """LowpassFilterBlock(64) -> ArbitraryResamplerBlock(48000 / 44100) -> ComplexMagnitudeBlock as one Chain equals the blocks run one by one, bit for bit,
    through process, the ring and two time partitions; the resampler fuses with nothing and is one launch"""
    n = 50000
    x = rand(16, n, True)
    want = x
    for b in chain_blocks():
        want = b.process(want)
    step = am.step_of(48000 / 44100)
    assert want.dtype == np.float32 and len(want) == am.output_count(n, step)
    chain = lr.Chain(chain_blocks())
    assert same_bits(chain.process(x), want)
    alone = [lr.Chain([b]) for b in chain_blocks()]
    y = x
    for c in alone:
        y = c.process(y)
    assert alone[1].last_launches == 1 and chain.last_launches == sum(c.last_launches for c in alone)
    # the ring
    ring = lr.Chain(chain_blocks())
    ring.set_ring(3, 16384)
    cuts = [0, 1, 78, 4174, 20558, 36942, n]
    got = np.concatenate(list(ring.stream(x[a:b] for a, b in zip(cuts[:-1], cuts[1:]))))
    assert same_bits(got, want)
    # two time partitions: the second seeks to its start minus the halo (63 + 15 samples) and replays it
    part = lr.Chain(chain_blocks())
    assert part.halo() == 63 + 15
    a = 23457
    first = timeshard.run_partition(part, x, 0, a, align=1)
    second = timeshard.run_partition(part, x, a, n, align=1)
    assert len(first) == am.output_count(a, step) and same_bits(np.concatenate([first, second]), want)
    # ... and on the boundaries the chain's own alignment asks for
    first = timeshard.run_partition(part, x, 0, a)
    second = timeshard.run_partition(part, x, a, n)
    assert same_bits(np.concatenate([first, second]), want)


# ---- the stage through the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["48000/44100", "0.37", "1/16", "16", "1.0"])
def test_stage_facts(case):
    L = _lib.load()
    for cplx in (True, False):
        blk = resampler(case, cplx)
        size = 8 if cplx else 4
        assert L.lrhip_stage_input_size(blk.stage_handle()) == size and L.lrhip_stage_output_size(blk.stage_handle()) == size
        for n in (0, 1, 77, 4096, (1 << 40) + 3):
            assert blk.max_output(n) == ((n << 48) // blk.step) + 2
        # memory() = T - 1: the halo of a chain of the stage alone; behind it, a filter's memory counts step / 2^48 input samples per sample
        T = blk.num_taps
        assert lr.Chain([blk]).halo() == T - 1
        fir = make(lr.FIRFilterBlock, [np.ones(65, np.float32)], tp(cplx), use_fft=lr.block.fir_mode(False))
        assert lr.Chain([blk, fir]).halo() == math.ceil(T - 1 + 64 * blk.step / 2.0 ** 48)
        # rate() = step / 2^48 in lowest terms: a stage behind it sees whole samples every step / gcd(step, 2^48) chain inputs
        assert lr.Chain([blk, fir]).shard_align() == blk.step // math.gcd(blk.step, 1 << 48)
