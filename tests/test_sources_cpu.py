"""The generator sources without a GPU: the numpy restatements of tests/helpers/source_models.py (what the device is held to bit for bit in
tests/test_gpu_sources.py) against the reference's golden vectors and its literal loop, the Philox known answers, the statistics of the random
stream, and the host side of the two blocks - op strings, argument assertions, rejected parameters."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, sources, types
from tests import golden_util
from tests.helpers import source_models as sm

RATIOS = [0.0123456789, 0.125, 440 / 48000, 0.499999]
AMPLITUDE, OFFSET, PHASE = 1.5, -0.25, 0.3
LONG = 100000


def ulp_f32(x):
    return float(np.spacing(np.float32(x)))


def test_restatement_against_the_golden_vectors():
    """all 14 vectors of the reference's signal_spec, at its epsilon, no sample excluded"""
    doc = golden_util.load("signalsource_spec")
    assert doc["block"] == "SignalSource" and doc["epsilon"] == 2e-5 and len(doc["vectors"]) == 14
    seen = set()
    for v in doc["vectors"]:
        signal, frequency, rate, options = v["args"]
        want = v["outputs"][0]
        got = sm.signal_closed_form(signal, frequency, rate, options["amplitude"], options["phase"], options["offset"], 0, len(want))
        assert got.dtype == want.dtype and len(want) == 256
        err = golden_util.max_abs_err(got, want)
        print("%-90s %.3g" % (v["desc"], err))
        assert err <= doc["epsilon"], (v["desc"], err)
        seen.add(signal)
    assert seen == set(sm.SIGNALS)


@pytest.fixture(scope="module")
def reference_loops():
    """the literal loop, once per (signal, ratio)"""
    return {(s, r): sm.signal_reference_loop(s, r * 48000.0, 48000.0, AMPLITUDE, PHASE, OFFSET, LONG) for s in sm.SIGNALS for r in RATIOS}


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("signal", ["square", "triangle", "sawtooth"])
def test_piecewise_waveforms_against_the_literal_loop(reference_loops, signal, ratio):
    """within one Float32 ulp of |amplitude| + |offset| over 100 000 samples: no edge sample flips"""
    got = sm.signal_closed_form(signal, ratio * 48000.0, 48000.0, AMPLITUDE, PHASE, OFFSET, 0, LONG)
    err = golden_util.max_abs_err(got, reference_loops[signal, ratio])
    print(signal, ratio, err)
    assert err <= ulp_f32(abs(AMPLITUDE) + abs(OFFSET))


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("signal", ["cosine", "sine", "exponential"])
def test_trigonometric_waveforms_against_the_literal_loop(reference_loops, signal, ratio):
    """the reference takes cosf of a Float32 phase of up to 2 pi + 8192 omega: half an ulp of that phase, times the amplitude, is its own error"""
    got = sm.signal_closed_form(signal, ratio * 48000.0, 48000.0, AMPLITUDE, PHASE, OFFSET, 0, LONG)
    err = golden_util.max_abs_err(got, reference_loops[signal, ratio])
    bound = AMPLITUDE * ulp_f32(2 * np.pi + 8192 * 2 * np.pi * ratio) / 2 + 1e-6
    print(signal, ratio, err, bound)
    assert err <= bound


def test_constant_and_the_ignored_parameters():
    assert np.array_equal(sm.signal_closed_form("constant", 50, 1000, 2.5, 0.7, -0.5, 5, 100), np.full(100, 2.5, np.float32))
    assert np.array_equal(sm.signal_reference_loop("constant", 50, 1000, 2.5, 0.7, -0.5, 100), np.full(100, 2.5, np.float32))
    # the exponential ignores the offset (signal.lua:80-94)
    assert np.array_equal(sm.signal_closed_form("exponential", 50, 1000, 2.5, 0.7, -0.5, 0, 100), sm.signal_closed_form("exponential", 50, 1000, 2.5, 0.7, 0.0, 0, 100))


def test_restatement_is_closed_form_in_the_index():
    """samples [n0, n0 + m) do not depend on where the run started, up to and past 2^33 and across the uint64 wrap of n * step"""
    for signal in sm.SIGNALS:
        whole = sm.signal_closed_form(signal, 440.0, 48000.0, AMPLITUDE, PHASE, OFFSET, 0, 10000)
        assert np.array_equal(whole[4097:4097 + 100], sm.signal_closed_form(signal, 440.0, 48000.0, AMPLITUDE, PHASE, OFFSET, 4097, 100))
    t = sm.turns(0.499999, 1.0, 0.3, (1 << 33) + 5, 3)
    assert [int(v) for v in t] == [(sm.fx(0.3 / sm.TWO_PI) + ((1 << 33) + 5 + k) * sm.fx(0.499999)) % (1 << 64) for k in range(3)]
    assert sm.fx(0.25) == 1 << 62 and sm.fx(-0.25) == 3 << 62 and sm.fx(1.0) == 0 and sm.fx(1 - 2.0 ** -60) == 0


def test_restated_phasor_is_the_float64_closed_form_to_rounding():
    rng = np.random.default_rng(1)
    t = rng.integers(0, 1 << 64, 200000, dtype=np.uint64)
    c, s = sm.phasor_from_turns(t)
    a = 2 * np.pi * (t.astype(np.float64) * 2.0 ** -64)
    assert max(np.max(np.abs(c - np.cos(a))), np.max(np.abs(s - np.sin(a)))) < 3e-7


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w[0]) for w in sm.philox4x32_10(counter, key)) == want


def test_philox_word_stream_layout():
    seed = 0x123456789abcdef0
    w = sm.philox_words(seed, 0, 64)
    for b in (0, 1, 15):
        block = sm.philox4x32_10((b, 0, 0, 0), (seed & 0xffffffff, seed >> 32))
        assert [int(v[0]) for v in block] == [int(v) for v in w[4 * b:4 * b + 4]]
    assert np.array_equal(sm.philox_words(seed, 7, 30), w[7:37])
    # the counter's second word takes over at j >> 2 = 2^32
    j0 = (1 << 34) - 2
    hi = sm.philox_words(seed, j0, 4)
    assert [int(v) for v in hi[:2]] == [int(v[0]) for v in sm.philox4x32_10((0xffffffff, 0, 0, 0), (seed & 0xffffffff, seed >> 32))][2:]
    assert [int(v) for v in hi[2:]] == [int(v[0]) for v in sm.philox4x32_10((0, 1, 0, 0), (seed & 0xffffffff, seed >> 32))][:2]


N_STAT = 1 << 16


@pytest.mark.parametrize("seed", [0, 1, 0x123456789abcdef0])
def test_random_stream_statistics(seed):
    """5 sigma bounds at N = 2^16: mean of U(-1, 1) sigma = 1 / sqrt(3 N); variance sigma = sqrt(4 / 45 / N); correlations sigma = 1 / sqrt(N);
    a bit's mean sigma = 1 / (2 sqrt(N)); chi-square with 25 degrees of freedom 25 + 5 sqrt(50)"""
    x = sm.uniform_random("f32", -1.0, 1.0, seed, 0, N_STAT).astype(np.float64)
    assert x.min() >= -1.0 and x.max() <= 1.0
    assert abs(x.mean()) < 0.0113
    assert abs(x.var() - 1 / 3) < 0.0058
    assert abs(np.corrcoef(x[:-1], x[1:])[0, 1]) < 0.0195
    z = sm.uniform_random("cf32", -1.0, 1.0, seed, 0, N_STAT)
    assert z.dtype == np.complex64 and abs(z.real).max() <= 1.0 and abs(z.imag).max() <= 1.0
    assert abs(np.corrcoef(z.real.astype(np.float64), z.imag.astype(np.float64))[0, 1]) < 0.0195
    y = sm.uniform_random("f32", 10.0, 100.0, seed, 0, N_STAT)
    assert y.min() >= 10.0 and y.max() <= 100.0
    bits = sm.uniform_random("bit", 0, 1, seed, 0, N_STAT)
    assert set(np.unique(bits)) == {0, 1} and abs(bits.mean() - 0.5) < 0.0098
    letters = sm.uniform_random("byte", 65, 90, seed, 0, N_STAT)
    counts = np.bincount(letters, minlength=256)
    assert np.all(counts[65:91] > 0) and counts[:65].sum() == 0 and counts[91:].sum() == 0
    expect = N_STAT / 26
    assert float(np.sum((counts[65:91] - expect) ** 2 / expect)) < 60.4
    full = sm.uniform_random("byte", 0, 255, seed, 0, N_STAT)
    assert full.min() == 0 and full.max() == 255


def test_random_stream_depends_on_the_seed_and_the_index_alone():
    a = sm.uniform_random("f32", -1, 1, 5, 0, 1000)
    assert np.array_equal(a[123:], sm.uniform_random("f32", -1, 1, 5, 123, 877))
    assert not np.array_equal(a, sm.uniform_random("f32", -1, 1, 6, 0, 1000))
    z = sm.uniform_random("cf32", -1, 1, 5, 0, 500)
    assert np.array_equal(z.view(np.float32), a)               # re from w(2 n), im from w(2 n + 1)
    assert np.array_equal(z[77:], sm.uniform_random("cf32", -1, 1, 5, 77, 423))


# ---- the blocks' host side ------------------------------------------------------------------------------------------------------------------
def test_signal_source_block():
    src = lr.SignalSource("exponential", 250e3, 2e6)
    assert src.get_output_type() is types.ComplexFloat32 and src.get_rate() == 2e6 and src.chunk_size == 8192 and src.type_signatures[0][0] == []
    assert src.op() == "signalsource:signal=exponential:frequency=250000:rate=2000000:amplitude=1:phase=0:offset=0"
    src = lr.SignalSource("cosine", 100e3, 1e6, {"amplitude": 2.5, "phase": 0.7853981633974483, "offset": -0.5})
    assert src.get_output_type() is types.Float32
    assert src.op() == "signalsource:signal=cosine:frequency=100000:rate=1000000:amplitude=2.5:phase=0.78539816339744828:offset=-0.5"
    for v in (0.1, 1 / 3, 440 / 48000, 5e-324, 1e300):
        assert float(sources.signal_op("sine", v, 1.0).split("frequency=")[1].split(":")[0]) == v          # %.17g gives the double back
    for signal in sm.REAL_SIGNALS:
        assert lr.SignalSource(signal, 1, 2).get_output_type() is types.Float32
    assert lr.SignalSource("constant", 0, 1, {"amplitude": 0.0}).op().endswith("amplitude=0:phase=0:offset=0")


def test_signal_source_assertions():
    with pytest.raises(AssertionError, match=r"Missing argument #1 \(signal\)"):
        lr.SignalSource()
    with pytest.raises(AssertionError, match=r'Unsupported signal \("x"\)'):
        lr.SignalSource("x", 1, 2)
    with pytest.raises(AssertionError, match=r"Missing argument #2 \(frequency\)"):
        lr.SignalSource("sine")
    with pytest.raises(AssertionError, match=r"Missing argument #3 \(rate\)"):
        lr.SignalSource("sine", 1)


def test_uniform_random_source_block():
    src = lr.UniformRandomSource(types.ComplexFloat32, 1e6)
    assert src.get_output_type() is types.ComplexFloat32 and src.get_rate() == 1e6 and src.chunk_size == 8192
    assert src.op() == "uniformrandomsource:type=cf32:lo=-1:hi=1:seed=0"
    assert lr.UniformRandomSource(types.Float32, 1e6, [10, 100], {"seed": 42}).op() == "uniformrandomsource:type=f32:lo=10:hi=100:seed=42"
    byte = lr.UniformRandomSource(types.Byte, 1e3)
    assert byte.get_output_type() is types.Byte and byte.op() == "uniformrandomsource:type=byte:lo=0:hi=255:seed=0"
    assert lr.UniformRandomSource(types.Byte, 1e3, [65, 90]).op() == "uniformrandomsource:type=byte:lo=65:hi=90:seed=0"
    bit = lr.UniformRandomSource(types.Bit, 1e3, [3, 9], {"seed": (1 << 64) - 1})
    assert bit.get_output_type() is types.Bit and bit.op() == "uniformrandomsource:type=bit:lo=0:hi=1:seed=18446744073709551615"


def test_uniform_random_source_assertions():
    with pytest.raises(AssertionError, match=r"Missing argument #1 \(data_type\)"):
        lr.UniformRandomSource()
    with pytest.raises(AssertionError, match=r"Missing argument #2 \(rate\)"):
        lr.UniformRandomSource(types.Float32)
    with pytest.raises(AssertionError, match="Unsupported data type"):
        lr.UniformRandomSource(types.RDSFrameType, 1.0)
    with pytest.raises(AssertionError, match="seed"):
        lr.UniformRandomSource(types.Float32, 1.0, None, {"seed": 1 << 64})


GOOD_SIGNAL = "signalsource:signal=sine:frequency=1:rate=2:amplitude=1:phase=0:offset=0"
REJECTED = [
    ("signalsource", "missing parameter \"signal\""),
    ("signalsource:signal=sine:frequency=1:rate=2:amplitude=1:phase=0", "missing parameter \"offset\""),
    (GOOD_SIGNAL + ":offset=1", "given twice"),
    (GOOD_SIGNAL + ":gain=1", "unknown parameter \"gain\""),
    (GOOD_SIGNAL + ":offset", "malformed"),
    ("signalsource:=sine:frequency=1:rate=2:amplitude=1:phase=0:offset=0", "malformed"),
    (GOOD_SIGNAL.replace("signal=sine", "signal=noise"), "Unsupported signal (\"noise\")"),
    (GOOD_SIGNAL.replace("rate=2", "rate=0"), "rate must be positive"),
    (GOOD_SIGNAL.replace("rate=2", "rate=-1"), "rate must be positive"),
    (GOOD_SIGNAL.replace("frequency=1", "frequency=inf"), "bad value for \"frequency\""),
    (GOOD_SIGNAL.replace("amplitude=1", "amplitude=nan"), "bad value for \"amplitude\""),
    (GOOD_SIGNAL.replace("phase=0", "phase=1e999"), "bad value for \"phase\""),
    (GOOD_SIGNAL.replace("offset=0", "offset=0x"), "bad value for \"offset\""),
    (GOOD_SIGNAL.replace("offset=0", "offset="), "bad value for \"offset\""),
    ("uniformrandomsource:type=f32:lo=-1:hi=1", "missing parameter \"seed\""),
    ("uniformrandomsource:type=f32:lo=-1:hi=1:seed=0:seed=1", "given twice"),
    ("uniformrandomsource:type=f32:lo=-1:hi=1:seed=0:range=1", "unknown parameter \"range\""),
    ("uniformrandomsource:type=f64:lo=-1:hi=1:seed=0", "unsupported type \"f64\""),
    ("uniformrandomsource:type=f32:lo=1:hi=-1:seed=0", "lo must not exceed hi"),
    ("uniformrandomsource:type=f32:lo=-inf:hi=1:seed=0", "bad value for \"lo\""),
    ("uniformrandomsource:type=f32:lo=-1e308:hi=1e308:seed=0", "hi - lo must be finite"),
    ("uniformrandomsource:type=byte:lo=-1:hi=10:seed=0", "0 .. 255"),
    ("uniformrandomsource:type=byte:lo=0:hi=256:seed=0", "0 .. 255"),
    ("uniformrandomsource:type=byte:lo=0.5:hi=10:seed=0", "0 .. 255"),
    ("uniformrandomsource:type=byte:lo=90:hi=65:seed=0", "lo must not exceed hi"),
    ("uniformrandomsource:type=f32:lo=-1:hi=1:seed=-1", "bad value for \"seed\""),
    ("uniformrandomsource:type=f32:lo=-1:hi=1:seed=1.5", "bad value for \"seed\""),
    ("uniformrandomsource:type=f32:lo=-1:hi=1:seed=18446744073709551616", "bad value for \"seed\""),
    ("uniformrandomsource:type=f32:lo=-1:hi=1:seed=", "bad value for \"seed\""),
]


@pytest.mark.parametrize("op,message", REJECTED)
def test_op_string_rejected(op, message):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    assert message in L.lrhip_strerror().decode(), L.lrhip_strerror().decode()
