"""PulseAmplitudeModulatorBlock and QuadratureAmplitudeModulatorBlock without a GPU: the model (tests/helpers/modulator_model.py) against the
reference's golden vectors, the blocks' default tables and argument checks, the op strings, and the loopback chains of the GPU tests decoded
by float64 models."""
import numpy as np
import pytest

from luaradio_amd import blocks as B
from tests import golden_util
from tests.helpers import digital_model as dm
from tests.helpers import modulator_loopback as lb
from tests.helpers import modulator_model as mm

RATE = 2.0


def golden_cases(name, option, default_table, dtype):
    for v in golden_util.load(name)["vectors"]:
        symbol_rate, sample_rate, count = v["args"][:3]
        options = v["args"][3] if len(v["args"]) > 3 else {}
        assert all(isinstance(o, (list, bool)) for o in options.values())           # plain data, never a Lua expression
        table = default_table(count)
        if option in options:
            table = np.array([complex(*e) if isinstance(e, list) else e for e in options[option]]).astype(dtype)
        yield v, table, int(np.floor(sample_rate / symbol_rate)), options.get("msb_first", True), options


def run_models(table, period, msb_first, x):
    bits = int(np.log2(len(table)))
    want = mm.literal_process([], x, table, bits, period, msb_first)
    state, parts = [], []
    for i in range(len(x)):
        parts.append(mm.literal_process(state, x[i:i + 1], table, bits, period, msb_first))
    fast = mm.ModulatorModel(table, period, msb_first)
    ragged = [fast.process(x[:1]), fast.process(x[1:100]), fast.process(x[100:100]), fast.process(x[100:])]
    return want, np.concatenate(parts), np.concatenate(ragged)


def test_golden_pam_model_zero_ulp():
    """the golden amplitudes are the Float32 values printed with 8 decimals; float32(text) gives them back, so the comparison is exact"""
    n = 0
    for v, table, period, msb_first, _ in golden_cases("pulseamplitudemodulator_spec", "amplitudes", mm.pam_table, np.float32):
        x, want = np.asarray(v["inputs"][0], np.uint8), v["outputs"][0]
        for got in run_models(table, period, msb_first, x):
            assert got.dtype == np.float32 and np.array_equal(got, want)
        n += 1
    assert n == 5


def test_golden_qam_model_zero_ulp():
    """0 ulp as well: scalar_div rounds each component once from double, which qam_table restates"""
    n = 0
    for v, table, period, msb_first, _ in golden_cases("quadratureamplitudemodulator_spec", "constellation", mm.qam_table, np.complex64):
        x, want = np.asarray(v["inputs"][0], np.uint8), v["outputs"][0]
        for got in run_models(table, period, msb_first, x):
            assert got.dtype == np.complex64 and np.array_equal(got, want)
        n += 1
    assert n == 6


def test_fast_model_equals_literal_with_junk_bytes():
    rng = np.random.default_rng(5)
    for bits, period, msb_first in [(1, 1, True), (3, 5, False), (4, 2, True), (8, 3, False)]:
        table = rng.standard_normal(1 << bits).astype(np.float32)
        x = mm.random_bits(rng, 1000)
        assert set(np.unique(x)) >= {0, 1, 2, 255}
        state, fast, pos = [], mm.ModulatorModel(table, period, msb_first), 0
        for n in [0, 1, bits - 1, bits, bits + 1, 63, 400]:
            a = mm.literal_process(state, x[pos:pos + n], table, bits, period, msb_first)
            assert np.array_equal(a, fast.process(x[pos:pos + n])) and list(fast.state) == state
            pos += n


@pytest.mark.parametrize("count", [2, 4, 8, 16, 64, 256])
def test_default_tables_equal_model(count):
    pam = B.PulseAmplitudeModulatorBlock(1.0, 4.0, count)
    qam = B.QuadratureAmplitudeModulatorBlock(1.0, 4.0, count)
    assert pam.table().dtype == np.float32 and np.array_equal(pam.table(), mm.pam_table(count))
    assert qam.table().dtype == np.complex64 and np.array_equal(qam.table(), mm.qam_table(count))
    assert (pam.symbol_bits, pam.symbol_period, pam.msb_first) == (int(np.log2(count)), 4, True)
    # unit mean energy
    assert abs(float(np.mean(pam.table().astype(np.float64) ** 2)) - 1) < 1e-6


def test_op_string_keeps_the_table_exactly():
    rng = np.random.default_rng(6)
    amps = rng.standard_normal(8).astype(np.float32) * np.float32(1e-3)
    blk = B.PulseAmplitudeModulatorBlock(1.0, 3.7, 8, {"amplitudes": list(amps), "msb_first": False})
    head, period, bits, msb, table = blk.op().split(":")
    assert (head, period, bits, msb) == ("pam", "period=3", "bits=3", "msb=0")
    assert np.array_equal(np.array([float(t) for t in table[len("table="):].split(",")]).astype(np.float32), amps)
    qam = B.QuadratureAmplitudeModulatorBlock(1.0, 2.0, 4, {"constellation": {0: (-1, -1), 1: -1 + 1j, 3: (1, -1), 2: 1 + 1j}})
    assert np.array_equal(qam.table(), np.array([-1 - 1j, -1 + 1j, 1 + 1j, 1 - 1j], np.complex64))
    assert qam.op() == "qam:period=2:bits=2:msb=1:table=-1,-1,-1,1,1,1,1,-1"


def test_signatures():
    from luaradio_amd import types
    pam, qam = B.PulseAmplitudeModulatorBlock(1.0, 2.0, 2), B.QuadratureAmplitudeModulatorBlock(1.0, 2.0, 2)
    pam.differentiate([types.Bit])
    qam.differentiate([types.Bit])
    assert pam.get_output_type() is types.Float32 and qam.get_output_type() is types.ComplexFloat32
    with pytest.raises(TypeError):
        pam.differentiate([types.Float32])


@pytest.mark.parametrize("cls", [B.PulseAmplitudeModulatorBlock, B.QuadratureAmplitudeModulatorBlock])
def test_assertions(cls):
    for bad in (0, 1, 3, 6, 12, 2.5, -4):
        with pytest.raises(AssertionError):
            cls(1.0, 2.0, bad)
    with pytest.raises(AssertionError):
        cls(None, 2.0, 2)
    with pytest.raises(AssertionError):
        cls(1.0, 2.0, None)
    with pytest.raises(ValueError, match="below one sample"):
        cls(2.0, 1.0, 2)                      # P = floor(0.5) = 0
    with pytest.raises(ValueError, match="2\\^16"):
        cls(1.0, 2.0, 1 << 17)
    option = "amplitudes" if cls is B.PulseAmplitudeModulatorBlock else "constellation"
    for incomplete in ({0: 1.0, 1: 2.0, 3: 4.0}, [1.0, 2.0, 3.0]):
        blk = cls(1.0, 2.0, 4, {option: incomplete})
        with pytest.raises(ValueError, match="no entry for symbol value"):
            blk.initialize()                  # refused before the library is asked for anything


def test_loopback_qam16_model_decodes_every_bit():
    period, table, sent = 8, mm.qam_table(16), lb.bits(lb.QAM_SEED)
    h = lb.rrc(period)
    y = mm.hold_fir_f64(mm.hold_fir_f64(mm.ModulatorModel(table, period).process(sent), h), h)
    delay, first = lb.qam_receiver_delay(period)
    peak, gain = lb.pulse_peak(period)
    assert (peak, delay, first) == (131, 5, 17)
    sampled = np.concatenate([np.zeros(delay), y])[:len(y)][::period][first:] / gain          # DelayBlock emits as many samples as it takes in
    dist = np.sort(np.abs(sampled[:, None] - table[None, :].astype(np.complex128)), axis=1)
    assert float(np.min(dist[:, 1] - dist[:, 0])) > 1e-2          # every decision is far from a tie: Float32 rounding cannot flip one
    decoded = lb.symbols_to_bits(lb.nearest_points(sampled, table), 4)
    # 1000 symbols go in; the first comes out as sample `first` = 17 of the 1000 behind the downsampler, the last 17 are still inside the filters
    assert len(decoded) == lb.NBITS - 4 * first and np.array_equal(decoded, sent[:len(decoded)])


def test_loopback_pam2_model_decodes_every_bit():
    period, table, sent = 16, mm.pam_table(2), lb.bits(lb.PAM_SEED)
    h = lb.rrc(period)
    y = mm.hold_fir_f64(mm.hold_fir_f64(mm.ModulatorModel(table, period).process(sent), h), h).astype(np.float32)
    decoded = dm.ClockSamplerModel(float(period), 0.0, 0.0).process(y)
    # the first decisions are taken before the first symbol's pulse peak (sample 136 = 8.5 symbols): a lag of 8 .. 10 bits, the same for all bits
    lag = lb.find_lag(decoded, sent, lb.pulse_peak(period)[0] // period)
    assert lag == 9 and len(decoded) - lag >= lb.NBITS - 12
