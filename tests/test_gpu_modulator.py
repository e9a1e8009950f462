"""PulseAmplitudeModulatorBlock and QuadratureAmplitudeModulatorBlock on the MI355X, bit for bit against the model
(tests/helpers/modulator_model.py): the reference's golden vectors, random bits in ragged chunks, seek, chains and the ring, a modulator -> pulse-shaping filter chain against
the separate blocks, and two noise-free loopback chains."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests import golden_util
from tests.helpers import modulator_loopback as lb
from tests.helpers import modulator_model as mm

pytestmark = pytest.mark.gpu

BLOCKS = {"pam": (lr.PulseAmplitudeModulatorBlock, "amplitudes", mm.pam_table, np.float32),
          "qam": (lr.QuadratureAmplitudeModulatorBlock, "constellation", mm.qam_table, np.complex64)}


def make(cls, args, in_type, rate=1.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def modulator(kind, bits, period, msb_first=True, table=None):
    """(block, model) of one modulator with 2^bits symbols and `period` samples per symbol"""
    cls, option, default_table, _ = BLOCKS[kind]
    options = {"msb_first": msb_first}
    if table is not None:
        options[option] = list(table)
    blk = make(cls, [1.0, float(period), 1 << bits, options], types.Bit)
    return blk, mm.ModulatorModel(default_table(1 << bits) if table is None else table, period, msb_first)


def custom_table(kind, bits, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(1 << bits).astype(np.float32)
    return t if kind == "pam" else (t + 1j * rng.standard_normal(1 << bits).astype(np.float32)).astype(np.complex64)


@pytest.mark.parametrize("kind", ["pam", "qam"])
def test_golden(kind):
    cls, option, default_table, dtype = BLOCKS[kind]
    name = "pulseamplitudemodulator_spec" if kind == "pam" else "quadratureamplitudemodulator_spec"
    vectors = golden_util.load(name)["vectors"]
    assert len(vectors) == (5 if kind == "pam" else 6)
    for v in vectors:
        args = list(v["args"])
        if len(args) > 3 and option in args[3]:
            args[3] = {option: [tuple(e) if isinstance(e, list) else e for e in args[3][option]]}
        x, want = np.asarray(v["inputs"][0], np.uint8), v["outputs"][0]
        whole, samplewise = golden_util.run_whole_and_samplewise(lambda: make(cls, args, types.Bit, rate=2.0), x)
        assert whole.dtype == dtype
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want), v["desc"]


# every b in {1, 2, 3, 4, 8, 16} and every P in {1, 2, 3, 5, 7, 64, 1000, 5003}, both bit orders, default and custom tables, both blocks; the 16-bit
# tables are read from global memory, the others from LDS
RANDOM_CASES = [("pam", 1, 1, True, False), ("qam", 2, 1, False, False), ("pam", 3, 1, True, True), ("qam", 4, 1, True, False),
                ("pam", 8, 1, False, True), ("qam", 16, 1, True, True), ("pam", 16, 2, False, False), ("qam", 1, 2, True, True),
                ("pam", 2, 3, False, True), ("qam", 3, 3, True, False), ("pam", 4, 5, True, False), ("qam", 8, 5, False, True),
                ("pam", 1, 7, False, True), ("qam", 2, 7, True, False), ("pam", 3, 64, True, False), ("qam", 4, 64, False, True),
                ("pam", 2, 1000, True, True), ("qam", 1, 1000, False, False), ("pam", 4, 5003, False, False), ("qam", 16, 5003, True, False)]


@pytest.mark.parametrize("kind,bits,period,msb_first,custom", RANDOM_CASES)
def test_random_bits_ragged_chunks(kind, bits, period, msb_first, custom):
    """every chunk's output and its length against max_output; bytes 2 and 255 count as 0; reset() drops the pending bits.  The big chunk is 4097
    symbols and a bit, cut to what gives about 2^22 output samples (839 symbols at P = 5003): still more than one workgroup per symbol and
    several symbols per call."""
    blk, model = modulator(kind, bits, period, msb_first, custom_table(kind, bits, 100 + bits) if custom else None)
    rng = np.random.default_rng(1000 * bits + period)
    big = min(4097, (1 << 22) // period + 1) * bits + 1
    chunks = [0, 1, bits - 1, bits, bits + 1, 63, big]
    for round_ in range(2):
        for n in chunks:
            x = mm.random_bits(rng, n)
            got, want = blk.process(x), model.process(x)
            assert got.dtype == want.dtype and len(got) <= blk.max_output(n) == -(-n // bits) * period
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (round_, n)
        # leave bits pending (unless b = 1), then reset: the next symbol starts at the next bit
        while bits > 1 and len(model.state) == 0:
            x = mm.random_bits(rng, 1)
            assert np.array_equal(blk.process(x), model.process(x))
        blk.reset()
        model.reset()
        chunks = [bits + 1, bits - 1, 1, 5 * bits]


def test_unaligned_output_buffer():
    """an output that does not start on 16 bytes (a piece of a long host call) takes the one-sample-per-thread kernel"""
    import torch
    L = _lib.load()
    rng = np.random.default_rng(3)
    for kind, bits, period in (("pam", 3, 5), ("qam", 2, 1), ("pam", 2, 1), ("qam", 4, 7)):
        blk, model = modulator(kind, bits, period)
        x = mm.random_bits(rng, 3001)
        want = model.process(x)
        words = want.dtype.itemsize // 4
        xt = torch.from_numpy(x).cuda()
        yt = torch.zeros(len(want) * words + 8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for off in (1, 2, 3) if kind == "pam" else (1,):
            blk.reset()
            n = blk.process_device(xt.data_ptr(), len(x), yt.data_ptr() + 4 * off * words, len(want))
            L.lrhip_synchronize()
            got = yt.cpu().numpy()[off * words:][:len(want) * words]
            assert n == len(want) and np.array_equal(got.view(np.uint32), want.view(np.float32).view(np.uint32)), (kind, off)


@pytest.mark.parametrize("kind,bits,period", [("pam", 3, 5), ("qam", 4, 1), ("qam", 2, 1000)])
def test_seek(kind, bits, period):
    blk, model = modulator(kind, bits, period)
    x = mm.random_bits(np.random.default_rng(4), 600 * bits)
    want = model.process(x)
    cuts = [0, 7 * bits, 100 * bits, 333 * bits, len(x)]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        blk.process(mm.random_bits(np.random.default_rng(a), bits + 1))     # another partition's state, pending bits included
        blk.seek(a)
        parts.append(blk.process(x[a:b]))
        assert len(parts[-1]) == (b - a) // bits * period
    assert np.array_equal(np.concatenate(parts), want)
    if bits > 1:
        blk.reset()
        first = blk.process(x[:bits + 1])
        with pytest.raises(lr.LrhipError, match="inside a symbol"):
            blk.seek(100 * bits + 1)
        # the refused seek changed nothing: the pending bit is still there
        assert np.array_equal(np.concatenate([first, blk.process(x[bits + 1:])]), want)
    chain = lr.Chain([blk])
    chain.seek(7 * bits)
    assert np.array_equal(chain.process(x[7 * bits:]), want[7 * period:])
    # a time partition of a chain starts between two symbols, and needs no replayed input
    assert chain.shard_align() == bits and chain.halo() == 0


def ragged(n, rng, pieces=7):
    cuts = np.sort(rng.integers(0, n + 1, pieces - 1))
    return list(zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]])))


def test_chains_and_ring():
    """PAM -> FrequencyModulator and QAM -> FrequencyTranslator: the Chain and the ring equal the separate blocks, chunk by chunk"""
    rng = np.random.default_rng(8)
    for kind, bits, period, tail_cls, tail_args, tail_in in (("pam", 2, 5, lr.FrequencyModulatorBlock, [0.25], types.Float32),
                                                            ("qam", 4, 3, lr.FrequencyTranslatorBlock, [0.1], types.ComplexFloat32)):
        x = mm.random_bits(rng, 40001)
        sep_mod, model = modulator(kind, bits, period)
        held = sep_mod.process(x)
        assert np.array_equal(held, model.process(x))
        want = make(tail_cls, tail_args, tail_in).process(held)
        mod, _ = modulator(kind, bits, period)
        chain = lr.Chain([mod, make(tail_cls, tail_args, tail_in)])
        assert chain.in_type is types.Bit
        got = np.concatenate([chain.process(x[a:b]) for a, b in ragged(len(x), rng)])
        assert np.array_equal(got, want)
        mod, _ = modulator(kind, bits, period)
        ring = lr.Chain([mod, make(tail_cls, tail_args, tail_in)])
        ring.set_ring(3, 9000)
        sizes = [9000, 1, 8999, 4097, 9000, 7903, 1001]
        assert sum(sizes) == len(x)
        parts = list(ring.stream(x[sum(sizes[:k]):sum(sizes[:k + 1])] for k in range(len(sizes))))
        assert np.array_equal(np.concatenate(parts), want)


def test_device_graph():
    g = lr.DeviceGraph()
    src = g.input("bits", types.Bit, rate=1.0)
    mod = lr.QuadratureAmplitudeModulatorBlock(1.0, 4.0, 16)
    g.connect(src, mod, lr.ComplexToRealBlock())
    g.initialize()
    x = mm.random_bits(np.random.default_rng(9), 4003)
    out = g.process(bits=x)
    (got,) = out.values()
    assert np.array_equal(got, mm.ModulatorModel(mm.qam_table(16), 4).process(x).real)


def shaped_blocks(kind, bits, period, num_taps, down):
    """modulator -> RootRaisedCosineFilterBlock [-> DownsamplerBlock(2)] at `period` samples per symbol"""
    mod, model = modulator(kind, bits, period)
    blocks = [mod, make(lr.RootRaisedCosineFilterBlock, [num_taps, 0.35, 1.0], mod.get_output_type(), rate=float(period))]
    if down:
        blocks.append(make(lr.DownsamplerBlock, [2], mod.get_output_type(), rate=float(period)))
    return blocks, model


def test_shaped_chain_equals_separate_blocks():
    """modulator -> RootRaisedCosineFilter [-> Downsampler] as a Chain that keeps every block's arithmetic, in ragged chunks, bit for bit"""
    rng = np.random.default_rng(10)
    x = mm.random_bits(rng, 8 * 3000 + 5)
    for kind, bits, period, down in (("qam", 2, 8, False), ("pam", 3, 3, True)):
        blocks, _ = shaped_blocks(kind, bits, period, 129, down)
        want = x
        for b in blocks:
            want = b.process(want)
        for flags in (_lib.CHAIN_NO_FUSION, _lib.CHAIN_NO_POLYPHASE_TAIL, _lib.CHAIN_EXACT):
            blocks, _ = shaped_blocks(kind, bits, period, 129, down)
            chain = lr.Chain(blocks, exact=flags)
            got = np.concatenate([chain.process(x[a:b]) for a, b in ragged(len(x), rng)])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, flags)


def test_loopback_qam16():
    """QAM(16), 8 samples per symbol -> RRC(129, 0.35) -> the same RRC -> Delay / Downsampler(8) on the pulse peak -> nearest constellation point:
    every one of the 4000 bits whose symbol comes out (the first is sample 17 behind the downsampler, so the last 17 symbols are still inside the
    filters and the delay)"""
    period, table, sent = 8, mm.qam_table(16), lb.bits(lb.QAM_SEED)
    delay, first = lb.qam_receiver_delay(period)
    _, gain = lb.pulse_peak(period)
    mod = make(lr.QuadratureAmplitudeModulatorBlock, [lb.SYMBOL_RATE, period * lb.SYMBOL_RATE, 16], types.Bit)
    cf, rate = types.ComplexFloat32, period * lb.SYMBOL_RATE
    chain = lr.Chain([mod, make(lr.RootRaisedCosineFilterBlock, [lb.RRC_TAPS, lb.RRC_BETA, lb.SYMBOL_RATE], cf, rate),
                      make(lr.RootRaisedCosineFilterBlock, [lb.RRC_TAPS, lb.RRC_BETA, lb.SYMBOL_RATE], cf, rate),
                      make(lr.DelayBlock, [delay], cf, rate), make(lr.DownsamplerBlock, [period], cf, rate)])
    sampled = chain.process(sent)[first:] / gain
    decoded = lb.symbols_to_bits(lb.nearest_points(sampled, table), 4)
    assert first == 17 and len(decoded) == lb.NBITS - 4 * first
    assert int(np.count_nonzero(decoded != sent[:len(decoded)])) == 0


def test_loopback_pam2_into_clock_sampler_and_slicer():
    """PAM(2), 16 samples per symbol -> RRC -> RRC -> ClockSamplerBlock -> SlicerBlock: the receiver blocks get back every bit at one fixed lag"""
    period, sent = 16, lb.bits(lb.PAM_SEED)
    f32, rate = types.Float32, period * lb.SYMBOL_RATE
    mod = make(lr.PulseAmplitudeModulatorBlock, [lb.SYMBOL_RATE, rate, 2], types.Bit)
    chain = lr.Chain([mod, make(lr.RootRaisedCosineFilterBlock, [lb.RRC_TAPS, lb.RRC_BETA, lb.SYMBOL_RATE], f32, rate),
                      make(lr.RootRaisedCosineFilterBlock, [lb.RRC_TAPS, lb.RRC_BETA, lb.SYMBOL_RATE], f32, rate),
                      make(lr.ClockSamplerBlock, [lb.SYMBOL_RATE], f32, rate), make(lr.SlicerBlock, [], f32, rate)])
    decoded = chain.process(sent)
    assert decoded.dtype == np.uint8
    lag = lb.find_lag(decoded, sent, lb.pulse_peak(period)[0] // period)
    assert lag is not None and len(decoded) - lag >= lb.NBITS - 12
