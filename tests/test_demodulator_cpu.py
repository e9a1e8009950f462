"""PulseAmplitudeDemodulatorBlock and QuadratureAmplitudeDemodulatorBlock without a GPU: the literal loop of the contract against its array form
(tests/helpers/demodulator_models.py), grid detection, the grid form against the general form, modulator model -> demodulator model, the blocks'
arguments and op strings, and the output count of any chunking."""
import numpy as np
import pytest

from luaradio_amd import blocks as B
from luaradio_amd import types
from tests.helpers import demodulator_models as dm
from tests.helpers import modulator_model as mm


def psk8():
    return np.exp(2j * np.pi * np.arange(8) / 8).astype(np.complex64)


def random_table(bits, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(1 << bits) + 1j * rng.standard_normal(1 << bits)).astype(np.complex64)


def noisy(rng, table, n, sigma=0.3):
    """n samples around random points of the table (complex or real as the table is)"""
    pts = np.asarray(table)[rng.integers(0, len(table), n)]
    if np.iscomplexobj(pts):
        return (pts + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return (pts + sigma * rng.standard_normal(n)).astype(np.float32)


def grid_midpoints(table, qb):
    """every pair (I midpoint or level, Q midpoint or level) of a grid table: samples exactly between neighbouring levels of either axis"""
    def marks(axis):
        lv = np.sort(np.unique(axis.astype(np.float32)))
        mid = ((lv[:-1].astype(np.float64) + lv[1:].astype(np.float64)) / 2).astype(np.float32)
        return np.concatenate([lv, mid])
    i, q = marks(table.real[::1 << qb]), marks(table.imag[:1 << qb])
    return (i[:, None] + 1j * q[None, :]).astype(np.complex64).reshape(-1)


# ---------------------------------------------------------------------------------------------------- the two models
MODEL_CASES = [("pam", mm.pam_table(4), 0), ("qam-grid", mm.qam_table(16), 2), ("qam-general", mm.qam_table(16), None), ("psk8", psk8(), None),
               ("qam32-grid", mm.qam_table(32), 2)]


@pytest.mark.parametrize("name,table,grid", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
@pytest.mark.parametrize("soft", [False, True])
def test_literal_loop_equals_array_model(name, table, grid, soft):
    rng = np.random.default_rng(len(table) + 7 * soft)
    x = noisy(rng, table, 60)
    x[7], x[11] = np.nan, np.inf
    for msb_first in (True, False):
        for period in (1, 3, 8):
            for offset in (0, period - 1):
                fast, pos = dm.DemodulatorModel(table, period, offset, msb_first, soft, 0.75, grid), 0
                for n in (0, 1, 2, 5, 1, 30, 21):
                    a = dm.literal_process(pos, x[pos:pos + n], table, period, offset, msb_first, soft, 0.75, grid)
                    g = fast.process(x[pos:pos + n])
                    assert a.dtype == g.dtype and (dm.same_floats(a, g) if soft else np.array_equal(a, g)), (msb_first, period, offset, pos, n)
                    pos += n
                assert pos == len(x) == fast.pos


def test_non_finite_samples_decide_symbol_zero():
    for table, grid in ((mm.qam_table(16), 2), (mm.qam_table(16), None), (mm.pam_table(4), 0)):
        x = np.array([np.nan, np.inf, -np.inf]).astype(table.dtype)
        if np.iscomplexobj(table):
            x = np.array([complex(np.nan, np.inf), complex(np.inf, np.nan), complex(-np.inf, -np.inf)], np.complex64)
        assert np.array_equal(dm.decide(x, table, grid, False, 1.0), [0, 0, 0])
        assert np.isnan(dm.decide(x, table, grid, True, 1.0)).all()
    # the grid form decides each axis on its own: a NaN real part is index 0 of the first axis, the second axis is decided as ever
    table = mm.qam_table(16)
    x = np.array([complex(np.nan, table[3].imag)], np.complex64)
    assert dm.decide(x, table, 2, False, 1.0)[0] == 3 and table[3].real == table[0].real and dm.decide(x, table, None, False, 1.0)[0] == 0


# ---------------------------------------------------------------------------------------------------- grid detection
@pytest.mark.parametrize("bits", range(2, 11))
def test_grid_detection_default_constellations(bits):
    table = B.qam_constellation(1 << bits)
    assert np.array_equal(table, mm.qam_table(1 << bits))
    qb = bits - (bits + 1) // 2
    assert dm.detect_grid(table) == qb and B.constellation_grid_bits(table) == qb
    # scaling keeps the grid: equal entries stay equal
    assert B.constellation_grid_bits(B.scaled_symbol_table(table, 0.3711)) == qb
    blk = B.QuadratureAmplitudeDemodulatorBlock(1.0, 1.0, 1 << bits, {"scale": 1.7})
    assert blk.grid() == qb and ":grid=%d:" % qb in blk.op() and ":grid=-1:" in blk.op(grid=-1)


def test_grid_detection_rejects_other_tables():
    for table in (psk8(), random_table(4, 1), random_table(7, 2)):
        assert dm.detect_grid(table) is None and B.constellation_grid_bits(table) is None
    blk = B.QuadratureAmplitudeDemodulatorBlock(1.0, 1.0, 8, {"constellation": list(psk8())})
    assert blk.grid() == -1 and ":grid=-1:" in blk.op()
    # one moved point of a grid is enough
    table = mm.qam_table(16).copy()
    table[5] = np.complex64(complex(table[5].real, np.nextafter(table[5].imag, np.float32(2))))
    assert dm.detect_grid(table) is None and B.constellation_grid_bits(table) is None
    # a real-valued constellation is a grid whose second axis has one entry
    assert dm.detect_grid(mm.pam_table(8).astype(np.complex64)) == 0
    big = B.QuadratureAmplitudeDemodulatorBlock(1.0, 1.0, 1 << 13, {"constellation": list(random_table(13, 3))})
    with pytest.raises(ValueError, match="2\\^12"):
        big.op()


# ---------------------------------------------------------------------------------------------------- the two forms
@pytest.mark.parametrize("bits", [2, 4, 5, 6, 8])
def test_soft_grid_form_equals_general_form(bits):
    table = dm.scaled_table(mm.qam_table(1 << bits), 0.8125)
    qb = dm.detect_grid(table)
    rng = np.random.default_rng(bits)
    x = np.concatenate([noisy(rng, table, 3000, 0.25), grid_midpoints(table, qb)])
    grid, general = dm.decide(x, table, qb, True, 1.25), dm.decide(x, table, None, True, 1.25)
    assert np.array_equal(grid.view(np.uint32), general.view(np.uint32))
    hard_grid, hard_general = dm.decide(x, table, qb, False, 1.0), dm.decide(x, table, None, False, 1.0)
    differ = np.flatnonzero(hard_grid != hard_general)
    print("QAM-%d: %d of %d hard decisions differ between the forms, all at samples %s" % (1 << bits, len(differ), len(x), differ[:8]))
    assert not np.any(differ < 3000)              # none on the random samples
    # where the forms differ, both candidates are at the same distance after the final addition: a tie of the general rule
    t = np.asarray(table, np.complex64)
    for s in differ:
        d = dm.decide(x[s:s + 1], table, None, True, 1.0)           # (the llr of any bit in which the two candidates differ is 0)
        k = [j for j in range(bits) if (hard_grid[s] ^ hard_general[s]) >> j & 1]
        assert np.all(d[0, k] == 0), (s, x[s], t[hard_grid[s]], t[hard_general[s]])


def test_soft_sign_is_the_hard_bit():
    rng = np.random.default_rng(21)
    for table, grid in ((mm.qam_table(64), 3), (mm.qam_table(64), None), (psk8(), None), (mm.pam_table(8), 0)):
        x = noisy(rng, table, 2000)
        llr, hard = dm.decide(x, table, grid, True, 2.0), dm.decide(x, table, grid, False, 1.0)
        bits = (hard[:, None] >> np.arange(llr.shape[1])) & 1
        assert np.array_equal((llr < 0)[llr != 0], bits.astype(bool)[llr != 0])


# ---------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("bits", range(1, 9))
def test_modulator_then_demodulator_is_the_identity(bits):
    rng = np.random.default_rng(30 + bits)
    sent = mm.random_bits(rng, 64 * bits, junk=False)
    cases = [(mm.pam_table(1 << bits), 0), (mm.qam_table(1 << bits), dm.detect_grid(mm.qam_table(1 << bits))), (mm.qam_table(1 << bits), None),
             (random_table(bits, 40 + bits), None), (rng.permutation(mm.pam_table(1 << bits)), 0)]
    for table, grid in cases:
        for msb_first in (True, False):
            for period in (1, 3):
                held = mm.ModulatorModel(table, period, msb_first).process(sent)
                got = dm.DemodulatorModel(table, period, 0, msb_first, False, 1.0, grid).process(held)
                assert np.array_equal(got, sent), (bits, grid, msb_first, period)
                llr = dm.DemodulatorModel(table, period, 0, msb_first, True, 1.0, grid).process(held)
                assert np.array_equal(llr < 0, sent.astype(bool)) and not np.any(llr == 0)


# ---------------------------------------------------------------------------------------------------- the blocks
def test_op_string_keeps_the_scaled_table_exactly():
    rng = np.random.default_rng(6)
    amps = rng.standard_normal(8).astype(np.float32) * np.float32(1e-3)
    scale = 1.0 / 3.0
    blk = B.PulseAmplitudeDemodulatorBlock(1.0, 3.7, 8, {"amplitudes": list(amps), "msb_first": False, "offset": 2, "scale": scale, "soft": True,
                                                         "noise_variance": 0.3})
    head, period, offset, bits, msb, soft, weight, grid, table = blk.op().split(":")
    assert (head, period, offset, bits, msb, soft, grid) == ("pamdemod", "period=3", "offset=2", "bits=3", "msb=0", "soft=1", "grid=1")
    want = (amps.astype(np.float64) * scale).astype(np.float32)
    assert np.array_equal(np.array([float(t) for t in table[len("table="):].split(",")]).astype(np.float32), want)
    assert np.array_equal(want, dm.scaled_table(amps, scale)) and np.array_equal(blk.received_table(), want)
    assert np.float32(float(weight[len("weight="):])) == np.float32(1.0 / 0.3) == blk.weight
    qam = B.QuadratureAmplitudeDemodulatorBlock(1.0, 2.0, 4, {"constellation": {0: (-1, -1), 1: -1 + 1j, 3: (1, -1), 2: 1 + 1j}, "scale": 0.5})
    # (value 2 = (I[1], Q[0]) would be 1 - 1j: this ordering is no grid)
    assert qam.op() == "qamdemod:period=2:offset=0:bits=2:msb=1:soft=0:weight=1:grid=-1:table=-0.5,-0.5,-0.5,0.5,0.5,0.5,0.5,-0.5"
    qam = B.QuadratureAmplitudeDemodulatorBlock(1.0, 2.0, 4, {"constellation": [-1 - 1j, -1 + 1j, 1 - 1j, 1 + 1j], "msb_first": False})
    assert qam.op() == "qamdemod:period=2:offset=0:bits=2:msb=0:soft=0:weight=1:grid=1:table=-1,-1,-1,1,1,-1,1,1"
    table = B.qam_constellation(64)
    q64 = B.QuadratureAmplitudeDemodulatorBlock(1.0, 1.0, 64, {"scale": 0.123})
    sent = np.array([float(t) for t in q64.op().split("table=")[1].split(",")]).astype(np.float32)
    assert np.array_equal(sent.view(np.complex64), dm.scaled_table(table, 0.123))
    # the modulators' op strings are what they were
    assert B.QuadratureAmplitudeModulatorBlock(1.0, 2.0, 4, {"constellation": [-1 - 1j, -1 + 1j, 1 + 1j, 1 - 1j]}).op() == \
        "qam:period=2:bits=2:msb=1:table=-1,-1,-1,1,1,1,1,-1"
    assert B.PulseAmplitudeModulatorBlock(1.0, 3.0, 2).op() == "pam:period=3:bits=1:msb=1:table=-1,1"


def test_signatures():
    pam, qam = B.PulseAmplitudeDemodulatorBlock(1.0, 2.0, 2), B.QuadratureAmplitudeDemodulatorBlock(1.0, 2.0, 4)
    pam.differentiate([types.Float32])
    qam.differentiate([types.ComplexFloat32])
    assert pam.get_output_type() is types.Bit and qam.get_output_type() is types.Bit
    with pytest.raises(TypeError):
        pam.differentiate([types.ComplexFloat32])
    with pytest.raises(TypeError):
        qam.differentiate([types.Bit])
    pam, qam = B.PulseAmplitudeDemodulatorBlock(1.0, 2.0, 2, {"soft": True}), B.QuadratureAmplitudeDemodulatorBlock(1.0, 2.0, 4, {"soft": True})
    pam.differentiate([types.Float32])
    qam.differentiate([types.ComplexFloat32])
    assert pam.get_output_type() is types.Float32 and qam.get_output_type() is types.Float32
    import luaradio_amd as lr
    assert lr.PulseAmplitudeDemodulatorBlock is B.PulseAmplitudeDemodulatorBlock and lr.QuadratureAmplitudeDemodulatorBlock is B.QuadratureAmplitudeDemodulatorBlock


@pytest.mark.parametrize("cls", [B.PulseAmplitudeDemodulatorBlock, B.QuadratureAmplitudeDemodulatorBlock])
def test_assertions(cls):
    """the modulators' assertions and texts (tests/test_modulator_cpu.py::test_assertions), and the demodulators' own options"""
    for bad in (0, 1, 3, 6, 12, 2.5, -4):
        with pytest.raises(AssertionError, match="is not greater than 1 and a power of 2"):
            cls(1.0, 2.0, bad)
    with pytest.raises(AssertionError, match="Missing argument #1 \\(symbol_rate\\)"):
        cls(None, 2.0, 2)
    with pytest.raises(AssertionError, match="Missing argument #2 \\(sample_rate\\)"):
        cls(1.0, None, 2)
    with pytest.raises(AssertionError, match="Missing argument #3"):
        cls(1.0, 2.0, None)
    with pytest.raises(ValueError, match="below one sample"):
        cls(2.0, 1.0, 2)
    with pytest.raises(ValueError, match="2\\^16"):
        cls(1.0, 2.0, 1 << 17)
    option = "amplitudes" if cls is B.PulseAmplitudeDemodulatorBlock else "constellation"
    for incomplete in ({0: 1.0, 1: 2.0, 3: 4.0}, [1.0, 2.0, 3.0]):
        blk = cls(1.0, 2.0, 4, {option: incomplete})
        with pytest.raises(ValueError, match="no entry for symbol value"):
            blk.initialize()                  # refused before the library is asked for anything
    for offset in (-1, 4, 1.5, True):
        with pytest.raises(ValueError, match="offset"):
            cls(1.0, 4.0, 4, {"offset": offset})
    assert cls(1.0, 4.0, 4, {"offset": 3}).offset == 3 and cls(1.0, 4.0, 4).offset == 0
    for nv in (0, -1.0, float("nan"), 1e-60, float("inf")):
        with pytest.raises(ValueError, match="noise_variance"):
            cls(1.0, 4.0, 4, {"soft": True, "noise_variance": nv})
    with pytest.raises(ValueError, match="needs soft"):
        cls(1.0, 4.0, 4, {"noise_variance": 2.0})
    with pytest.raises(ValueError, match="scale"):
        cls(1.0, 4.0, 4, {"scale": float("inf")})
    blk = cls(1.0, 4.0, 4, {"soft": True, "noise_variance": 0.1})
    assert blk.weight.dtype == np.float32 and blk.weight == np.float32(1.0 / 0.1) and blk.msb_first is True and blk.symbol_period == 4


# ---------------------------------------------------------------------------------------------------- counting
def test_output_count_of_any_chunking_and_of_seek():
    rng = np.random.default_rng(50)
    table = mm.pam_table(4)
    for period, offset in ((1, 0), (3, 0), (3, 2), (8, 5), (8, 7)):
        x = noisy(rng, table, 200)
        whole = dm.DemodulatorModel(table, period, offset).process(x)
        assert len(whole) == 2 * len(range(offset, len(x), period))
        for sizes in ([1] * len(x), [0, 2, 1, 7, 0, 64, 3, 123], list(rng.integers(0, 12, 60))):
            m, pos, parts = dm.DemodulatorModel(table, period, offset), 0, []
            for n in sizes:
                n = int(min(n, len(x) - pos))
                parts.append(m.process(x[pos:pos + n]))
                # the symbols whose sample s P + offset lies in [pos, pos + n), counted one by one; never more than max_output = (n / P + 1) b
                assert len(parts[-1]) == 2 * sum(1 for s in range(len(x)) if pos <= s * period + offset < pos + n) <= (n // period + 1) * 2
                pos += n
            assert np.array_equal(np.concatenate(parts), whole[:len(np.concatenate(parts))])
        for n0 in (0, 1, offset, offset + 1, period, 5 * period + offset - 1, 5 * period + offset, 5 * period + offset + 1, 199):
            n0 = max(n0, 0)
            m = dm.DemodulatorModel(table, period, offset)
            emitted = m.seek(n0)
            first = 0 if n0 <= offset else -(-(n0 - offset) // period)
            assert emitted == 2 * first == 2 * sum(1 for s in range(len(x)) if s * period + offset < n0)
            assert np.array_equal(m.process(x[n0:]), whole[emitted:])


# ---------------------------------------------------------------------------------------------------- the library's own checks
GOOD = "qamdemod:period=2:offset=1:bits=2:msb=1:soft=0:weight=1:grid=1:table=-1,-1,-1,1,1,-1,1,1"
OP_REFUSALS = [(GOOD.replace("period=2", "period=0"), "period must be 1 .. 2^30 - 1"),
               (GOOD.replace("period=2", "period=1073741824"), "period must be 1 .. 2^30 - 1"),
               (GOOD.replace("offset=1", "offset=2"), "offset must be 0 .. period - 1"),
               (GOOD.replace("offset=1", "offset=-1"), "offset must be 0 .. period - 1"),
               (GOOD.replace("bits=2", "bits=17"), "bits per symbol must be 1 .. 16"),
               (GOOD.replace("msb=1", "msb=2"), "msb must be 0 or 1"),
               (GOOD.replace("soft=0", "soft=2"), "soft must be 0 or 1"),
               (GOOD.replace("weight=1", "weight=0"), "weight must be"),
               (GOOD.replace("weight=1", "weight=1e60"), "weight must be"),
               (GOOD.replace("weight=1", "weight=x"), "bad value for \"weight\""),
               (GOOD.replace("grid=1", "grid=3"), "grid must be -1"),
               (GOOD.replace("grid=1", "grid=-2"), "grid must be -1"),
               (GOOD.replace("grid=1", "grid=0"), "the table is no grid with 0 low bits"),
               (GOOD.replace("1,-1,1,1", "1,1,1,-1"), "the table is no grid with 1 low bits: entry 1 is not"),
               (GOOD.replace(":grid=1", ""), "missing parameter \"grid\""),
               (GOOD.replace(":offset=1", ""), "missing parameter \"offset\""),
               (GOOD + ",", "the table ends with a comma"),
               (GOOD + ",1", "the table has 9 values, 2 bits per symbol need 8"),
               (GOOD.replace("msb=1", "gain=1"), "unknown parameter \"gain\""),
               ("qamdemod:period=1:offset=0:bits=13:msb=1:soft=0:weight=1:grid=-1:table=" + ",".join(["0.5"] * (2 << 13)), "limited to 12 bits per symbol"),
               ("pamdemod:period=1:offset=0:bits=1:msb=1:soft=0:weight=1:grid=-1:table=-1,1", "grid must be 1"),
               ("pamdemod:period=1:offset=0:bits=1:msb=1:soft=0:weight=1:grid=1:table=-1,1,2", "the table has 3 values, 1 bits per symbol need 2")]


@pytest.mark.parametrize("op, fragment", OP_REFUSALS, ids=[str(i) for i in range(len(OP_REFUSALS))])
def test_defective_op_strings_are_refused_in_front_of_the_device(op, fragment):
    from luaradio_amd import _lib
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith(op.split(":")[0] + ":") and fragment in message, message
