"""PulseAmplitudeDemodulatorBlock and QuadratureAmplitudeDemodulatorBlock on the MI355X, bit for bit against the model
(tests/helpers/demodulator_models.py; a NaN LLR - inf - inf for a non-finite sample - matches any NaN): ragged chunks, decision boundaries, soft against
hard, seek and time partitions, pointers off 16 bytes, guard words, the modulator tests' loopback chains with the decision on the device, a DeviceGraph
and the ring.

A workgroup decides 256 symbols (one per lane), 512 (qam) or 1024 (pam) with period 1 on a 16-byte aligned input, where a lane takes the symbols of one
16-byte load: the streams are three such tiles and 5 symbols long."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, timeshard, types
from tests.helpers import demodulator_models as dm
from tests.helpers import guarded as GD
from tests.helpers import modulator_loopback as lb
from tests.helpers import modulator_model as mm
from tests.test_gpu_bounds import TorchMemory, device_call

pytestmark = pytest.mark.gpu

PERIODS = [(1, 0), (3, 2), (8, 5)]


def psk8():
    return np.exp(2j * np.pi * np.arange(8) / 8).astype(np.complex64)


def random_table(bits, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(1 << bits) + 1j * rng.standard_normal(1 << bits)).astype(np.complex64)


def tile(kind, period):
    """symbols per workgroup (stage_demodulator.h: DEM_NT lanes of PER symbols)"""
    return 256 * ((4 if kind == "pam" else 2) if period == 1 else 1)


def demodulator(kind, bits, period, offset, msb_first=True, soft=False, table=None, general=False, scale=1.0, noise_variance=None, rate=None):
    """(block, model): `general` runs a grid-shaped table through the general search (grid=-1)"""
    cls = lr.PulseAmplitudeDemodulatorBlock if kind == "pam" else lr.QuadratureAmplitudeDemodulatorBlock
    options = {"msb_first": msb_first, "offset": offset, "soft": soft, "scale": scale}
    if table is not None:
        options["amplitudes" if kind == "pam" else "constellation"] = list(table)
    if noise_variance is not None:
        options["noise_variance"] = noise_variance
    blk = cls(1.0, float(period), 1 << bits, options)
    blk.rate = float(period) if rate is None else rate
    blk.differentiate([types.Float32 if kind == "pam" else types.ComplexFloat32])
    if general:
        blk._set_stage(_lib.load().lrhip_unary_create(blk.op(grid=-1).encode(), 0.0, 0.0, 0, 0), "Creating a qamdemod stage with grid=-1")
    else:
        blk.initialize()
    if table is None:
        table = mm.pam_table(1 << bits) if kind == "pam" else mm.qam_table(1 << bits)
    received = dm.scaled_table(table, scale)
    grid = 0 if kind == "pam" else (None if general else dm.detect_grid(received))
    assert blk.grid() == (1 if kind == "pam" else -1 if grid is None else grid) or general
    weight = np.float32(1.0 / (1.0 if noise_variance is None else noise_variance))
    return blk, dm.DemodulatorModel(received, period, offset, msb_first, soft, weight, grid)


def noisy(rng, table, n, sigma=0.3):
    pts = np.asarray(table)[rng.integers(0, len(table), n)]
    if np.iscomplexobj(pts):
        return (pts + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return (pts + sigma * rng.standard_normal(n)).astype(np.float32)


def same(got, want, soft):
    return got.dtype == want.dtype and (dm.same_floats(got, want) if soft else np.array_equal(got, want))


def ragged(n, period):
    """call lengths that add up to n: empty and one-sample calls, calls shorter than a symbol, calls that emit nothing, two large ones"""
    sizes = [0, 1, 1, max(period - 1, 1), period, 2, 5 * period + 1, 1]
    big = (n - sum(sizes) - 3) // 2
    sizes += [big, 1, 2, n - sum(sizes) - big - 3]
    assert sum(sizes) == n and min(sizes) >= 0
    return sizes


# kind, bits, msb_first, table, general
CASES = {"pam2": ("pam", 1, True, None, False), "pam4": ("pam", 2, False, None, False), "pam8": ("pam", 3, True, None, False),
         "qam4": ("qam", 2, False, None, False), "qam16": ("qam", 4, True, None, False), "qam32": ("qam", 5, False, None, False),
         "qam64": ("qam", 6, True, None, False), "qam256": ("qam", 8, False, None, False), "psk8": ("qam", 3, True, psk8(), False),
         "random128": ("qam", 7, False, random_table(7, 70), False), "qam16-general": ("qam", 4, True, None, True)}


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("name", list(CASES))
def test_ragged_chunks_against_the_model(name, soft):
    kind, bits, msb_first, table, general = CASES[name]
    rng = np.random.default_rng(bits + 100 * soft)
    for period, offset in PERIODS:
        blk, model = demodulator(kind, bits, period, offset, msb_first, soft, table, general, scale=0.9, noise_variance=0.4 if soft else None)
        n = (3 * tile(kind, period) + 5) * period
        x = noisy(rng, model.table, n)
        pos, silent = 0, 0
        for size in ragged(n, period):
            got, want = blk.process(x[pos:pos + size]), model.process(x[pos:pos + size])
            assert len(got) <= blk.max_output(size) == (size // period + 1) * bits
            assert same(got, want, soft), (period, offset, pos, size, np.flatnonzero(got != want)[:4] if len(got) == len(want) else (len(got), len(want)))
            silent += size > 0 and len(got) == 0
            pos += size
        assert period == 1 or silent >= 2          # some calls emitted nothing
        blk.reset()
        model.reset()
        assert same(blk.process(x[:7 * period]), model.process(x[:7 * period]), soft)


def boundary_marks(levels):
    """the levels of one axis, every midpoint between neighbours, and the Float32 neighbours of each midpoint"""
    lv = np.sort(np.unique(np.asarray(levels, np.float32)))
    mid = ((lv[:-1].astype(np.float64) + lv[1:].astype(np.float64)) / 2).astype(np.float32)
    return np.concatenate([lv, mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))]).astype(np.float32)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("form", ["qam16-grid", "qam16-general", "pam4", "pam4-general"])
def test_decision_boundaries(form, soft):
    """samples on every midpoint between neighbouring levels and one ulp to either side, on each axis against every mark of the other one, then one NaN
    and one infinite sample.  pam4-general: the four amplitudes as a real-valued constellation through the general search."""
    if form.startswith("qam16"):
        table = mm.qam_table(16)
        i, q = boundary_marks(table.real), boundary_marks(table.imag)
        x = (i[:, None] + 1j * q[None, :]).astype(np.complex64).reshape(-1)
        blk, model = demodulator("qam", 4, 1, 0, True, soft, None, form.endswith("general"))
    elif form == "pam4":
        x = boundary_marks(mm.pam_table(4))
        blk, model = demodulator("pam", 2, 1, 0, True, soft)
    else:
        x = boundary_marks(mm.pam_table(4)).astype(np.complex64)
        blk, model = demodulator("qam", 2, 1, 0, True, soft, mm.pam_table(4).astype(np.complex64), True)
    tail = np.array([np.nan, np.inf], np.float32).astype(x.dtype)
    if np.iscomplexobj(x):
        tail = np.array([complex(np.nan, 0.1), complex(np.inf, -np.inf)], np.complex64)
    x = np.concatenate([x, tail])
    got, want = blk.process(x), model.process(x)
    assert same(got, want, soft), np.flatnonzero(got != want)[:8]
    bits = model.b
    if soft:
        assert np.isnan(got[-bits:]).all()
        assert np.any(got == 0)                    # a midpoint is a tie of at least one bit
    elif form != "qam16-grid":
        assert not got[-2 * bits:].any()           # the NaN and the infinite sample decide symbol 0
    else:
        assert not got[-bits:].any()               # (the grid form decides the finite axis of the NaN sample as ever)


@pytest.mark.parametrize("name", ["pam8", "qam64", "qam16-general", "psk8"])
def test_soft_sign_is_the_hard_bit(name):
    kind, bits, msb_first, table, general = CASES[name]
    rng = np.random.default_rng(bits)
    hard_blk, model = demodulator(kind, bits, 1, 0, msb_first, False, table, general)
    soft_blk, _ = demodulator(kind, bits, 1, 0, msb_first, True, table, general, noise_variance=0.05)
    x = noisy(rng, model.table, 3 * tile(kind, 1) + 5, 0.4)
    hard, llr = hard_blk.process(x), soft_blk.process(x)
    assert len(hard) == len(llr) == len(x) * bits and np.count_nonzero(llr) > len(llr) // 2
    assert np.array_equal((llr < 0)[llr != 0], hard.astype(bool)[llr != 0])


@pytest.mark.parametrize("kind,bits,period,offset,soft", [("qam", 4, 8, 5, False), ("pam", 2, 3, 2, True), ("qam", 3, 1, 0, True)])
def test_seek_and_time_partitions(kind, bits, period, offset, soft):
    table = psk8() if bits == 3 else None
    blk, model = demodulator(kind, bits, period, offset, True, soft, table)
    rng = np.random.default_rng(5)
    n = 700 * period
    x = noisy(rng, model.table, n)
    want = model.process(x)
    # any position: inside a symbol, on its sample, right behind it, before the first one
    for n0 in (0, 1, offset, offset + 1, period, 10 * period + offset - 1, 10 * period + offset, 10 * period + offset + 1, 333, n - 1, n):
        n0 = min(max(n0, 0), n)
        blk.process(x[:period + 1])                # another partition's position
        blk.seek(n0)
        first = 0 if n0 <= offset else -(-(n0 - offset) // period)
        assert same(blk.process(x[n0:]), want[first * bits:], soft), n0
    chain = lr.Chain([blk])
    assert chain.halo() == 0 and chain.shard_align() == 1
    cuts = sorted({0, 1, period + offset, 97, 98, 5 * period + offset + 1, 401, n})
    parts = [timeshard.run_partition(chain, x, a, b, align=1) for a, b in zip(cuts[:-1], cuts[1:])]
    assert same(np.concatenate(parts), want, soft)
    assert len(parts[0]) == (bits if offset == 0 else 0)


@pytest.mark.parametrize("kind,bits,period,soft", [("qam", 4, 1, False), ("qam", 3, 1, True), ("pam", 2, 1, False), ("pam", 3, 3, True), ("qam", 8, 1, False),
                                                   ("qam", 8, 1, True), ("qam", 4, 3, True), ("qam", 6, 1, True)])
def test_pointers_off_16_bytes(kind, bits, period, soft):
    """an input that does not start on 16 bytes takes the one-symbol-per-lane kernel, an output that is not aligned to b bytes the byte stores; LLRs
    leave in 16- or 8-byte stores only where the run of an axis' bits (4 + 4, 2 + 2, 3 + 3 here) and its address allow"""
    import torch
    table = psk8() if (kind, bits) == ("qam", 3) else None
    blk, model = demodulator(kind, bits, period, 0, True, soft, table)
    rng = np.random.default_rng(6)
    x = noisy(rng, model.table, (3 * tile(kind, period) + 5) * period)
    want = model.process(x)
    words = x.dtype.itemsize // 4
    out_size = 4 if soft else 1
    for in_off in (0, 1, 3):
        for out_off in (0, 1, 2, 5):
            xt = torch.zeros(len(x) * words + 8, dtype=torch.float32, device="cuda")
            xt[in_off * words:in_off * words + len(x) * words] = torch.from_numpy(x.view(np.float32)).cuda()
            yt = torch.zeros(len(want) * out_size + 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            blk.reset()
            count = blk.process_device(xt.data_ptr() + 4 * in_off * words, len(x), yt.data_ptr() + out_off * out_size, len(want))
            _lib.check(_lib.load().lrhip_synchronize(), "synchronize")
            raw = yt.cpu().numpy()
            got = raw[out_off * out_size:out_off * out_size + len(want) * out_size].copy().view(want.dtype)
            assert count == len(want) and same(got, want, soft), (in_off, out_off)
            assert not raw[:out_off * out_size].any() and not raw[out_off * out_size + len(want) * out_size:].any()


@pytest.mark.parametrize("name,period,offset,soft", [("qam16", 1, 0, False), ("qam16", 3, 2, True), ("pam4", 1, 0, True), ("psk8", 1, 0, False),
                                                     ("qam256", 8, 5, False)])
def test_guard_words(name, period, offset, soft):
    """tests/helpers/guarded.py, as tests/test_gpu_bounds.py runs it: nothing is written before the output or behind the count (max_output is the
    capacity), every output of the count is written, the input is untouched, and NaN words behind the call's n samples change nothing - nothing past n
    is read"""
    kind, bits, msb_first, table, general = CASES[name]
    t = tile(kind, period) * period
    pairs = [(2 * t + 1, 3), (3, 3 * t - 1), (3 * t, 1)]
    rng = np.random.default_rng(9)
    _, model = demodulator(kind, bits, period, offset, msb_first, soft, table, general)
    x = noisy(rng, model.table, max(sum(p) for p in pairs))
    mem = TorchMemory()
    for pair in pairs:
        model.reset()
        want = [model.process(x[:pair[0]]), model.process(x[pair[0]:sum(pair)])]
        for in_off in (0, 1):
            for out_off in (0, 1):
                def check(c, got):
                    assert same(got, want[c], soft), (pair, in_off, out_off, c)
                GD.run_guarded(lambda: demodulator(kind, bits, period, offset, msb_first, soft, table, general)[0], [x], list(pair), in_off, out_off, mem=mem,
                               call=device_call, max_output=lambda obj, n: obj.max_output(n), in_kind="float", out_dtype=np.float32 if soft else np.uint8,
                               out_floats=soft, check=check)


def make(cls, args, in_type, rate=1.0):
    blk = cls(*args)
    blk.rate = rate
    blk.differentiate([in_type])
    blk.initialize()
    return blk


@pytest.mark.parametrize("kind", ["qam", "pam"])
def test_loopback_decided_on_the_device(kind):
    """the chain of tests/test_gpu_modulator.py::test_loopback_qam16 (16 points; pam: 4 levels), 8 samples per symbol -> RRC -> RRC, and the decision on
    the device: behind Delay / Downsampler(8) with period 1, and in their place with period 8 and the pulse peak's offset.  Every bit whose symbol comes
    out is the one sent, over at least the span the host decision covers today, and the chain's output is Bit."""
    period, bits, sent = 8, 4 if kind == "qam" else 2, lb.bits(lb.QAM_SEED if kind == "qam" else lb.PAM_SEED)
    delay, first = lb.qam_receiver_delay(period)
    peak, gain = lb.pulse_peak(period)
    assert (peak, delay, first) == (131, 5, 17)
    mod_cls, dem_cls = (lr.QuadratureAmplitudeModulatorBlock, lr.QuadratureAmplitudeDemodulatorBlock) if kind == "qam" else \
        (lr.PulseAmplitudeModulatorBlock, lr.PulseAmplitudeDemodulatorBlock)
    st, rate = types.ComplexFloat32 if kind == "qam" else types.Float32, period * lb.SYMBOL_RATE

    def head():
        return [make(mod_cls, [lb.SYMBOL_RATE, rate, 1 << bits], types.Bit),
                make(lr.RootRaisedCosineFilterBlock, [lb.RRC_TAPS, lb.RRC_BETA, lb.SYMBOL_RATE], st, rate),
                make(lr.RootRaisedCosineFilterBlock, [lb.RRC_TAPS, lb.RRC_BETA, lb.SYMBOL_RATE], st, rate)]

    behind = lr.Chain(head() + [make(lr.DelayBlock, [delay], st, rate), make(lr.DownsamplerBlock, [period], st, rate),
                                make(dem_cls, [lb.SYMBOL_RATE, lb.SYMBOL_RATE, 1 << bits, {"scale": gain}], st, lb.SYMBOL_RATE)])
    in_place = lr.Chain(head() + [make(dem_cls, [lb.SYMBOL_RATE, rate, 1 << bits, {"scale": gain, "offset": peak % period}], st, rate)])
    for chain, skip in ((behind, first), (in_place, peak // period)):
        assert chain.in_type is types.Bit and chain.out_type is types.Bit
        out = chain.process(sent)
        assert out.dtype == np.uint8 and len(out) == (lb.NBITS // bits) * bits
        decoded = out[bits * skip:]
        assert len(decoded) >= lb.NBITS - bits * first
        assert int(np.count_nonzero(decoded != sent[:len(decoded)])) == 0


def test_device_graph():
    g = lr.DeviceGraph()
    src = g.input("samples", types.ComplexFloat32, rate=3.0)
    hard = lr.QuadratureAmplitudeDemodulatorBlock(1.0, 3.0, 16, {"offset": 1})
    soft = lr.QuadratureAmplitudeDemodulatorBlock(1.0, 3.0, 16, {"offset": 2, "soft": True, "msb_first": False})
    g.connect(src, lr.ComplexConjugateBlock(), hard)
    g.connect(src, soft)
    g.initialize()
    table = mm.qam_table(16)
    x = noisy(np.random.default_rng(9), table, 3 * 777 + 1)
    out = g.process(samples=x)
    got = {v.dtype: v for v in out.values()}
    assert len(out) == 2
    assert np.array_equal(got[np.dtype(np.uint8)], dm.DemodulatorModel(table, 3, 1, True, False, 1.0, 2).process(np.conj(x)))
    assert dm.same_floats(got[np.dtype(np.float32)], dm.DemodulatorModel(table, 3, 2, False, True, 1.0, 2).process(x))


def test_ring():
    """submit / collect: the chunks of a stream through a ring of three slots, the stage behind a MultiplyConstantBlock"""
    blk, model = demodulator("qam", 6, 3, 1, True, False, scale=2.0)
    gain = make(lr.MultiplyConstantBlock, [2.0], types.ComplexFloat32, 3.0)
    ring = lr.Chain([gain, blk])
    ring.set_ring(3, 4000)
    x = noisy(np.random.default_rng(10), mm.qam_table(64), 13001)
    want = model.process(gain.process(x))
    sizes = [4000, 1, 3999, 2, 1, 4000, 998]
    assert sum(sizes) == len(x)
    parts, pos = [], 0
    for size in sizes:
        if ring.in_flight == 3:
            parts.append(ring.collect())
        ring.submit(x[pos:pos + size])
        pos += size
    while ring.in_flight:
        parts.append(ring.collect())
    assert len(parts) == len(sizes) and any(len(p) == 0 for p in parts)
    assert np.array_equal(np.concatenate(parts), want)
