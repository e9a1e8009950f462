"""SignalSource and UniformRandomSource on the MI355X: the reference's golden vectors, long runs in ragged chunks and after seek() against the
restatements of tests/helpers/source_models.py (bit for bit where the arithmetic is exact double, to the translator's 1e-6 for the phasor), both
kernel forms inside guard words, and the sources as the head of a Chain - generate, the ring, time partitions, and what such a chain refuses."""
import ctypes as C
import tempfile

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import guarded as GD
from tests.helpers import source_models as sm

pytestmark = pytest.mark.gpu

RATE = 48000.0
RATIOS = [0.0123456789, 0.125, 440 / 48000, 0.499999]
AMPLITUDE, OFFSET, PHASE = 1.5, -0.25, 0.3
OPTIONS = {"amplitude": AMPLITUDE, "offset": OFFSET, "phase": PHASE}
EXACT_SIGNALS = ("square", "triangle", "sawtooth", "constant")
LONG = 300000
CHUNKS = [1, 77, 4096, 100000]
RANDOM = {"cf32": (types.ComplexFloat32, None, (-1.0, 1.0)), "f32": (types.Float32, [10, 100], (10.0, 100.0)),
          "byte": (types.Byte, [65, 90], (65, 90)), "bit": (types.Bit, None, (0, 1))}


def signal(name, ratio, options=OPTIONS):
    src = lr.SignalSource(name, ratio * RATE, RATE, options)
    src.initialize()
    return src


def random_source(kind, seed):
    data_type, rng, _ = RANDOM[kind]
    src = lr.UniformRandomSource(data_type, RATE, rng, {"seed": seed})
    src.initialize()
    return src


def make(cls, args, in_type, rate=RATE):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def chunked(src, total, chunks=CHUNKS):
    parts = [src.process(n) for n in chunks]
    parts.append(src.process(total - sum(chunks)))
    assert [len(p) for p in parts] == chunks + [total - sum(chunks)]
    return np.concatenate(parts)


def trig_tolerance(amplitude=AMPLITUDE, offset=OFFSET):
    """1e-6 |A|: the bar of the translator's test_rotator_vs_closed_form_long_and_chunked for the same phasor; 2^-23 (|A| + |O|): the one rounding
    of c A + O to Float32"""
    return 1e-6 * abs(amplitude) + 2.0 ** -23 * (abs(amplitude) + abs(offset))


def check_signal(name, ratio, got, n0):
    """samples [n0, n0 + len(got)) of the stream against the restatement"""
    if name in EXACT_SIGNALS:
        want = sm.signal_closed_form(name, ratio * RATE, RATE, AMPLITUDE, PHASE, OFFSET, n0, len(got))
        assert same_bits(got, want), (name, ratio, n0, int(np.argmax(got != want)))
    else:
        want = sm.signal_exact(name, ratio * RATE, RATE, AMPLITUDE, PHASE, 0.0 if name == "exponential" else OFFSET, n0, len(got))
        err = float(np.max(np.abs(got.astype(want.dtype) - want)))
        print("%-12s f/rate = %-22r n0 = %-12d max |error| = %.3g (bar %.3g)" % (name, ratio, n0, err, trig_tolerance()))
        assert err <= trig_tolerance(), (name, ratio, n0, err)


def test_stage_sizes_and_defaults():
    L = _lib.load()
    for name in sm.SIGNALS:
        src = signal(name, 0.125)
        assert L.lrhip_stage_input_size(src.stage_handle()) == 0
        assert L.lrhip_stage_output_size(src.stage_handle()) == (8 if name == "exponential" else 4)
        assert src.max_output(12345) == 12345
        out = src.process()
        assert len(out) == 8192 and out.dtype == (np.complex64 if name == "exponential" else np.float32)
        assert len(src.process(0)) == 0
    for kind, size in (("cf32", 8), ("f32", 4), ("byte", 1), ("bit", 1)):
        src = random_source(kind, 0)
        assert L.lrhip_stage_input_size(src.stage_handle()) == 0 and L.lrhip_stage_output_size(src.stage_handle()) == size
        assert len(src.process()) == 8192


def test_golden():
    doc = golden_util.load("signalsource_spec")
    assert len(doc["vectors"]) == 14 and doc["epsilon"] == 2e-5
    for v in doc["vectors"]:
        src = lr.SignalSource(*v["args"])
        src.initialize()
        got, want = src.process(256), v["outputs"][0]
        assert got.dtype == want.dtype
        err = golden_util.max_abs_err(got, want)
        print("%-90s %.3g" % (v["desc"], err))
        assert err <= doc["epsilon"], (v["desc"], err)


@pytest.mark.parametrize("name", sm.SIGNALS)
def test_long_run_chunked(name):
    for ratio in RATIOS:
        whole = signal(name, ratio).process(LONG)
        assert same_bits(chunked(signal(name, ratio), LONG), whole), (name, ratio)
        check_signal(name, ratio, whole, 0)
        src = signal(name, ratio)
        src.process(1000)
        src.reset()
        assert same_bits(src.process(5000), whole[:5000])


@pytest.mark.parametrize("name", sm.SIGNALS)
def test_seek(name):
    ratio, m = RATIOS[0], 10000
    whole = signal(name, ratio).process(4097 + m)
    src = signal(name, ratio)
    for n0 in (1, 4097):
        src.process(33)                                         # another partition's index
        src.seek(n0)
        assert same_bits(src.process(m), whole[n0:n0 + m]), (name, n0)
    # past 2^32, where no uncut run reaches: the restatement, and the same samples from a run that was cut elsewhere
    n0 = (1 << 33) + 5
    src.seek(n0)
    got = src.process(m)
    check_signal(name, ratio, got, n0)
    src.seek(n0 - 4099)
    assert same_bits(src.process(4099 + m)[4099:], got)
    chain = lr.Chain([src])
    chain.seek(n0)
    assert same_bits(chain.generate(m), got)
    assert chain.halo() == 0 and chain.shard_align() == 1


@pytest.mark.parametrize("seed", [0, 0x123456789abcdef0])
@pytest.mark.parametrize("kind", list(RANDOM))
def test_random_against_the_restatement(kind, seed):
    lo, hi = RANDOM[kind][2]
    whole = random_source(kind, seed).process(LONG)
    assert same_bits(whole, sm.uniform_random(kind, lo, hi, seed, 0, LONG))
    assert same_bits(chunked(random_source(kind, seed), LONG), whole)
    src = random_source(kind, seed)
    # 2^34 - 3: the second counter word takes over inside the call (cf32: at 2^33 - 3)
    for n0 in (1, 4097, (1 << 33) + 5, (1 << 33) - 3, (1 << 34) - 3):
        src.seek(n0)
        got = src.process(5001)
        assert same_bits(got, sm.uniform_random(kind, lo, hi, seed, n0, 5001)), (kind, n0)
        if n0 < LONG - 5001:
            assert same_bits(got, whole[n0:n0 + 5001])
    src.reset()
    assert same_bits(src.process(100), whole[:100])
    if kind in ("cf32", "f32"):
        v = whole.view(np.float32)
        assert v.min() >= lo and v.max() <= hi


def test_host_call_in_pieces():
    """a host call of 2^20 samples and more travels as pipelined pieces (chain.h host_execute): for a source they have no copy in, and the pieces
    are cuts of the stream like any other"""
    n = (1 << 21) + 5
    got = signal("sawtooth", RATIOS[0]).process(n)
    assert same_bits(got, sm.signal_closed_form("sawtooth", RATIOS[0] * RATE, RATE, AMPLITUDE, PHASE, OFFSET, 0, n))
    assert same_bits(random_source("cf32", 9).process(n), sm.uniform_random("cf32", -1.0, 1.0, 9, 0, n))
    chain = lr.Chain([random_source("bit", 9), make(lr.PulseAmplitudeModulatorBlock, [1.0, 1.0, 2], types.Bit)])
    assert same_bits(chain.generate(n), np.where(sm.uniform_random("bit", 0, 1, 9, 0, n) == 1, np.float32(1), np.float32(-1)))


# ---- both kernel forms inside guard words ----------------------------------------------------------------------------------------------------
# outputs of one workgroup: kernels_source.h source_vec_kernel covers 256 * SRC_U (= 4) stores of 16 bytes, source_scalar_kernel 256 samples
def tile(out_size, aligned):
    return 256 * 4 * (16 // out_size) if aligned else 256


BOUNDS_CASES = [("cosine", lambda: signal("cosine", RATIOS[2]), np.float32), ("square", lambda: signal("square", RATIOS[0]), np.float32),
                ("exponential", lambda: signal("exponential", RATIOS[1]), np.complex64), ("random f32", lambda: random_source("f32", 7), np.float32),
                ("random cf32", lambda: random_source("cf32", 7), np.complex64), ("random byte", lambda: random_source("byte", 7), np.uint8),
                ("random bit", lambda: random_source("bit", 7), np.uint8)]


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one sample off"])
@pytest.mark.parametrize("case", BOUNDS_CASES, ids=[c[0] for c in BOUNDS_CASES])
def test_bounds(case, aligned):
    """two consecutive calls of n samples into [guard | offset | payload | guard]: nothing before the pointer, nothing at or behind n samples, every
    sample written, and the values those of one uncut host call whatever the kernel form"""
    import torch
    _, factory, dtype = case
    size = np.dtype(dtype).itemsize
    T = tile(size, aligned)
    lens = [1, 3, 2 * T + 1, 2 * T + 2, 2 * T + 3, 3 * T - 1, 3 * T]
    want = factory().process(2 * max(lens))
    lo = GD.G + (0 if aligned else size)
    assert (lo % 16 == 0) == aligned
    nbytes = (lo + max(lens) * size + 3) // 4 * 4 + GD.G
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fill = torch.from_numpy(GD.sentinel_fill(nbytes))
    L = _lib.load()
    src = factory()
    for n in lens:
        src.reset()
        for call in range(2):
            buf.copy_(fill)
            torch.cuda.synchronize()
            assert src.process_device(buf.data_ptr() + lo, n) == n
            _lib.check(L.lrhip_synchronize(), "synchronize")
            y = buf.cpu().numpy()
            try:
                GD.check_before(y, lo)
                GD.check_after(y, lo, n * size)
                GD.check_written(y, lo, n * size, size, "<f4" if np.dtype(dtype).kind in "fc" else None)
            except GD.GuardViolation as e:
                raise GD.GuardViolation("n = %d, call %d: %s" % (n, call, e)) from None
            got = np.frombuffer(y[lo:lo + n * size].tobytes(), dtype)
            assert same_bits(got, want[call * n:(call + 1) * n]), (n, call)


def test_capacity_and_null_output_are_refused():
    import torch
    src = signal("sine", 0.125)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    L = _lib.load()
    assert L.lrhip_stage_execute_device(src.stage_handle(), None, 17, buf.data_ptr(), 16) < 0
    assert "output capacity 16 < 17" in _lib.last_error()
    assert L.lrhip_stage_execute_device(src.stage_handle(), None, 16, None, 16) < 0
    assert "null" in _lib.last_error()
    # nothing was generated: the index did not move
    assert same_bits(src.process(8), signal("sine", 0.125).process(8))
    # a stage that has an input still refuses a null one
    blk = make(lr.MultiplyConstantBlock, [2.0], types.Float32)
    assert L.lrhip_stage_execute_device(blk.stage_handle(), None, 16, buf.data_ptr(), 16) < 0
    assert "null buffer" in _lib.last_error()
    out = np.empty(16, np.float32)
    assert L.lrhip_stage_execute(blk.stage_handle(), None, 16, out.ctypes.data_as(C.c_void_p), 16) < 0
    assert "null input buffer" in _lib.last_error()


# ---- a source as the head of a chain ---------------------------------------------------------------------------------------------------------
def tail_blocks():
    return [make(lr.LowpassFilterBlock, [16, 8e3], types.Float32), make(lr.DownsamplerBlock, [5], types.Float32)]


def source_chain():
    return lr.Chain([signal("cosine", RATIOS[2])] + tail_blocks(), exact=True)


@pytest.fixture(scope="module")
def separate_blocks():
    """the source's own output fed through the blocks one by one, once"""
    x = signal("cosine", RATIOS[2]).process(20000)
    y = x
    for b in tail_blocks():
        y = b.process(y)
    return x, y


def test_chain_generate_equals_the_blocks_one_by_one(separate_blocks):
    x, want = separate_blocks
    chain = source_chain()
    assert chain.source and chain.in_type is None and chain.out_type is types.Float32
    assert chain.max_output(20000) >= 4000                      # a bound: the downsampler may emit one more in another phase
    got = chain.generate(20000)
    assert len(want) == 4000 and same_bits(got, want)
    # the source is a launch of its own: one more than the same blocks fed the samples
    fed = lr.Chain(tail_blocks(), exact=True)
    assert same_bits(fed.process(x), want)
    assert chain.last_launches == fed.last_launches + 1
    # the stream goes on where the call ended, and starts again after reset()
    more = chain.generate(5000)
    chain.reset()
    assert same_bits(np.concatenate([chain.generate(12345), chain.generate(12655)]), np.concatenate([got, more]))
    # on the device, with a null input pointer
    import torch
    chain.reset()
    out = torch.zeros(4000, dtype=torch.float32, device="cuda")
    assert chain.process_device(None, 20000, out.data_ptr(), 4000) == 4000
    _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
    assert same_bits(out.cpu().numpy(), want)


def test_chain_ring_equals_generate(separate_blocks):
    _, want = separate_blocks
    ring = source_chain()
    ring.set_ring(2, 8192)
    sizes = [8192, 1, 4096, 7711]
    assert sum(sizes) == 20000
    parts = list(ring.stream(sizes))
    assert len(parts) == len(sizes) and same_bits(np.concatenate(parts), want)
    ring.reset()
    assert ring.submit(5000) == 1000 and ring.submit(6808) == 1362 and ring.in_flight == 2          # samples 0, 5, .. 11805 of 11808
    assert same_bits(np.concatenate([ring.collect(), ring.collect()]), want[:2362])
    with pytest.raises(lr.LrhipError, match="exceeds the ring's max_chunk"):
        ring.submit(8193)


def test_chain_time_partitions(separate_blocks):
    _, want = separate_blocks
    probe = source_chain()
    align, halo = probe.shard_align(), probe.halo()
    print("shard_align", align, "halo", halo)
    assert align >= 1 and halo >= 15                            # the filter's 15 samples of history, at the least
    for boundary in (5 * align, 2000 * align, 2005 * align):
        first = source_chain()
        assert first.start_at(0) == 0
        a = first.generate(boundary)
        second = source_chain()
        s = second.start_at(boundary)
        assert s <= boundary - halo or s == 0
        assert s % align == 0
        b = second.generate(20000 - s)                          # the generated samples in front of `boundary` are the replayed halo: dropped
        assert same_bits(np.concatenate([a, b]), want), boundary


def test_chain_refusals():
    L = _lib.load()
    with pytest.raises(lr.LrhipError, match=r"stage 1 \(signalsource\) is a source and can only be the first stage"):
        lr.Chain([make(lr.MultiplyConstantBlock, [2.0], types.Float32), signal("cosine", 0.125)])
    with pytest.raises(lr.LrhipError, match=r"stage 1 \(uniformrandomsource\) is a source"):
        lr.Chain([signal("cosine", 0.125), random_source("f32", 0)])
    chain = source_chain()
    x = np.zeros(16, np.float32)
    with pytest.raises(TypeError, match="takes no input"):
        chain.process(x)
    with pytest.raises(TypeError, match="takes no input"):
        chain.push(x)
    chain.set_ring(2, 8192)
    with pytest.raises(TypeError, match="takes no input"):
        chain.submit(x)
    with pytest.raises(TypeError, match="takes no input"):
        chain.ring_input()
    out = np.empty(L.lrhip_chain_push_bound(chain._chain, 16), np.float32)
    assert L.lrhip_chain_push(chain._chain, x.ctypes.data_as(C.c_void_p), 16, out.ctypes.data_as(C.c_void_p), len(out)) < 0
    assert "lrhip_chain_push: the chain starts with a source (signalsource) and takes no input" in _lib.last_error()
    assert not L.lrhip_chain_ring_input(chain._chain)
    assert "lrhip_chain_ring_input: the chain starts with a source" in _lib.last_error()
    with tempfile.TemporaryFile() as f:
        f.write(bytes(4096))
        f.flush()
        with pytest.raises(lr.LrhipError, match="lrhip_chain_submit_fd: the chain starts with a source"):
            chain.submit_fd(f.fileno(), 0, 100)
    assert chain.in_flight == 0 and len(chain.flush()) == 0
    # the refusals left the chain as it was
    assert same_bits(chain.generate(100), source_chain().generate(100))
    # generate() is for chains without an input; a chain that has one still refuses a null input, on every path
    fed = lr.Chain(tail_blocks(), exact=True)
    with pytest.raises(TypeError, match="generate"):
        fed.generate(100)
    y = np.empty(100, np.float32)
    assert L.lrhip_chain_execute(fed._chain, None, 100, y.ctypes.data_as(C.c_void_p), 100) < 0
    assert "null input buffer" in _lib.last_error()
    fed.set_ring(2, 1000)
    assert L.lrhip_chain_submit(fed._chain, None, 100) < 0
    assert "null input buffer" in _lib.last_error()


def test_random_source_feeds_a_modulator_chain():
    """UniformRandomSource(Bit) -> PulseAmplitudeModulator: what a synthetic transmit graph starts with"""
    def blocks():
        return [random_source("bit", 3), make(lr.PulseAmplitudeModulatorBlock, [1.0, 4.0, 4], types.Bit)]
    bits = sm.uniform_random("bit", 0, 1, 3, 0, 4001)
    want = blocks()[1].process(bits)
    chain = lr.Chain(blocks())
    assert same_bits(np.concatenate([chain.generate(1001), chain.generate(3000)]), want)
    assert chain.shard_align() == 2 and chain.halo() == 0
