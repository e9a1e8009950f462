"""ArbitraryResamplerBlock without a device: the position arithmetic of luaradio_amd/csrc/arbresample_plan.h (tools/host_arbresample_check.hip, built for
the host) against Python's big integers where a 64-bit product overflows, the output counts of a stream cut into calls, the quality of the default
design on the f64 model (tests/helpers/arbresample_model.py), and the refusals of the block's options and of the op string, which need no device."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests.helpers import arbresample_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = [1 << 44, 1 << 52, int(np.rint(2.0 ** 48 * 44100 / 48000)), 1 << 48, (1 << 48) + 1]
BIG = [0, 1, (1 << 32) - 1, (1 << 40) + 3, (1 << 63) - 1]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/host_arbresample_check.hip as plain C++; returns ask(lines) -> the answers, one list of integers per line"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("arbcheck")
    exe = str(d / "host_arbresample_check")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tools", "host_arbresample_check.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    def ask(lines):
        listing = str(d / "cases.txt")
        with open(listing, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, listing], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = r.stdout.strip().split("\n")
        assert len(out) == len(lines) and all(o.split()[0] == ln.split()[0] for o, ln in zip(out, lines))
        return [[int(v) for v in o.split()[1:]] for o in out]
    return ask


def test_steps_are_what_the_block_computes():
    assert STEPS[0] == am.step_of(16.0) and STEPS[1] == am.step_of(1 / 16) and STEPS[2] == am.step_of(48000 / 44100) and STEPS[3] == am.step_of(1.0)
    for ratio in (48000 / 44100, 0.37, math.sqrt(2), 1 + 35e-6, 16.0, 1 / 8):
        blk = lr.ArbitraryResamplerBlock(ratio)
        assert blk.step == am.step_of(ratio) and (1 << 44) <= blk.step <= (1 << 52)
        assert blk.effective_ratio == 2.0 ** 48 / blk.step and abs(blk.effective_ratio / ratio - 1) <= 2.0 ** -45
        assert blk.num_taps == am.taps_per_phase(ratio) and len(blk.taps) == 64 * blk.num_taps
        assert np.array_equal(blk.taps, am.prototype(ratio))
        blk.rate = 44100.0
        assert blk.get_rate() == 44100.0 * blk.effective_ratio
    # at 1 / 16 the 16 taps per phase stretch to 256: 32 phases are the most that fit P * T <= 8192
    blk = lr.ArbitraryResamplerBlock(1 / 16, {"phases": 32})
    assert blk.num_taps == 256 and blk.step == STEPS[1] and np.array_equal(blk.taps, am.prototype(1 / 16, 32))
    assert lr.ArbitraryResamplerBlock(0.37).num_taps == 44


@pytest.mark.parametrize("log2p", [4, 6, 8])
def test_positions_where_64_bits_overflow(checker, log2p):
    cases = [(s, m) for s in STEPS for m in BIG]
    got = checker(["pos %d %d %d" % (s, log2p, m) for s, m in cases])
    for (s, m), (i_hi, i_lo, p, mu24) in zip(cases, got):
        assert ((i_hi << 64) | i_lo, p, mu24) == am.position(m, s, log2p), (s, m)
    # the pieces fit their types
    assert all(0 <= g[2] < (1 << log2p) and 0 <= g[3] < (1 << 24) for g in got)


def test_counts_where_64_bits_overflow(checker):
    cases = [(s, q) for s in STEPS for q in BIG]
    for what in ("count", "seek"):
        got = checker(["%s %d %d" % (what, s, q) for s, q in cases])
        for (s, q), (hi, lo) in zip(cases, got):
            assert (hi << 64) | lo == am.output_count(q, s), (what, s, q)
    got = checker(["max %d %d" % (s, q) for s, q in cases])
    for (s, q), (bound,) in zip(cases, got):
        assert bound == min(((q << 48) // s) + 2, (1 << 64) - 1), (s, q)
    # a count is the first m whose newest input has not arrived
    for s in STEPS:
        for q in (1, 77, 4175, (1 << 40) + 3):
            m = am.output_count(q, s)
            assert am.position(m, s, 6)[0] >= q and (m == 0 or am.position(m - 1, s, 6)[0] < q)


@pytest.mark.parametrize("step", STEPS)
def test_counts_of_a_cut_stream(checker, step):
    total = 10000
    chunks = [1, 1, 77, 0, 4096]
    chunks.append(total - sum(chunks))
    ends = np.cumsum(chunks).tolist()
    cum = [(hi << 64) | lo for hi, lo in checker(["count %d %d" % (step, q) for q in ends])]
    bounds = [b for (b,) in checker(["max %d %d" % (step, n) for n in chunks])]
    per_call = [c - b for c, b in zip(cum, [0] + cum[:-1])]
    assert all(0 <= n <= b for n, b in zip(per_call, bounds)), (per_call, bounds)
    assert sum(per_call) == am.output_count(total, step) and per_call[3] == 0
    assert cum == [am.output_count(q, step) for q in ends]


def test_most_single_sample_calls_return_nothing_when_decimating_by_16(checker):
    step = am.step_of(1 / 16)
    cum = [lo for _, lo in checker(["count %d %d" % (step, q) for q in range(1, 33)])]
    per_call = [c - b for c, b in zip(cum, [0] + cum[:-1])]
    assert per_call == ([1] + [0] * 15) * 2


# ---- the default design on the f64 model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [48000 / 44100, math.sqrt(2), 0.37, 16.0], ids=["48000/44100", "sqrt(2)", "0.37", "16"])
def test_quality_of_the_default_design(ratio):
    """a complex tone at 0.2 min(1, ratio) cycles per input sample: behind the first 4 T max(1, ratio) + 10 outputs, the output minus the best-fit multiple
    of the ideal tone delayed by (P T - 1) / (2 P) input samples has an rms of at most -55 dB of the tone, and the fitted gain is within 1 % of 1.
    (Measured on this model: -62.0 .. -62.1 dB at 48000/44100, sqrt(2) and 16, -73.8 dB at 0.37; gain 1.0031 .. 1.0034.  The bar leaves 7 dB for a
    change of window.)"""
    P, n = 64, 40000
    G, D, T, step = am.tables(ratio, P)
    f = 0.2 * min(1.0, ratio)
    x = np.exp(2j * np.pi * f * np.arange(n)).astype(np.complex64)
    y, _ = am.model_f64(x, G, D, step)
    assert len(y) == am.output_count(n, step)
    skip = int(4 * T * max(1.0, ratio) + 10)
    m = np.arange(skip, len(y))
    t = m.astype(np.float64) * (step / 2.0 ** 48) - (P * T - 1) / (2 * P)          # (m step < 2^53 * 2^11 here: exact enough, 2^-30 of a sample)
    ideal = np.exp(2j * np.pi * f * t)
    gain = np.vdot(ideal, y[skip:]) / np.vdot(ideal, ideal)
    err_db = 10 * np.log10(np.mean(np.abs(y[skip:] - gain * ideal) ** 2))
    print("ratio %-10.6g T = %-3d residual %.1f dB, gain %.4f%+.4fj" % (ratio, T, err_db, gain.real, gain.imag))
    assert err_db <= -55.0, err_db
    assert abs(gain - 1) <= 0.01, gain


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [((0,), "ratio"), ((float("nan"),), "ratio"), ((17,), "ratio"), ((1 / 17,), "ratio"),
                                        ((1.5, {"phases": 48}), "phases"), ((1.5, {"taps_per_phase": 5}), "taps_per_phase"),
                                        ((0.1, {"phases": 256}), "phases"), ((1.5, {"taps": np.zeros(64 * 16 - 1, np.float32)}), "taps")],
                         ids=["ratio 0", "ratio nan", "ratio 17", "ratio 1/17", "phases 48", "taps_per_phase 5", "P * T > 8192", "taps of the wrong length"])
def test_defective_options_are_refused(args, word):
    with pytest.raises((ValueError, AssertionError)) as e:
        lr.ArbitraryResamplerBlock(*args)
    assert str(e.value).startswith("arbresampler:") and word in str(e.value), str(e.value)


def test_accepted_options():
    assert lr.ArbitraryResamplerBlock(0.1, {"phases": 32}).num_taps == 160
    blk = lr.ArbitraryResamplerBlock(1.3, {"phases": 16, "taps_per_phase": 4, "taps": np.arange(64)})
    assert blk.taps.dtype == np.float32 and len(blk.taps) == 64
    blk.differentiate([types.Float32])
    assert blk.op().startswith("arbresampler:type=f32:phases=16:step=%d:taps=0,1,2," % am.step_of(1.3))


def _taps(n):
    return ",".join("%.9g" % (0.001 * (k % 17)) for k in range(n))


OP_REFUSALS = [("arbresampler:type=cf32:phases=64:step=%d:taps=%s:bogus=1" % (1 << 48, _taps(1024)), "unknown parameter \"bogus\""),
               ("arbresampler:type=cf32:phases=64:taps=%s" % _taps(1024), "missing parameter \"step\""),
               ("arbresampler:type=cf32:phases=64:step=%d:taps=%s" % (1 << 53, _taps(1024)), "step"),
               ("arbresampler:type=cf32:phases=64:step=%d:taps=%s" % ((1 << 44) - 1, _taps(1024)), "step"),
               ("arbresampler:type=cf32:phases=64:step=-5:taps=%s" % _taps(1024), "step"),
               ("arbresampler:type=cf32:phases=64:step=%d:taps=%s" % (1 << 48, _taps(1000)), "multiple of phases"),
               ("arbresampler:type=cf32:phases=48:step=%d:taps=%s" % (1 << 48, _taps(48 * 16)), "phases"),
               ("arbresampler:type=cf32:phases=64:step=%d:taps=%s" % (1 << 48, _taps(128)), "taps per phase"),
               ("arbresampler:type=cf32:phases=256:step=%d:taps=%s" % (1 << 48, _taps(256 * 34)), "must not exceed 8192"),
               ("arbresampler:type=s16:phases=64:step=%d:taps=%s" % (1 << 48, _taps(1024)), "type"),
               ("arbresampler:type=cf32:phases=64:step=%d:taps=" % (1 << 48), "multiple of phases")]


@pytest.mark.parametrize("op, fragment", OP_REFUSALS, ids=["unknown key", "no step", "step 2^53", "step 2^44 - 1", "step negative", "taps not a multiple of P",
                                                           "phases 48", "T = 2", "P * T > 8192", "type", "no taps"])
def test_defective_op_strings_are_refused_in_front_of_the_device(op, fragment):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 1)
    message = L.lrhip_strerror().decode()
    assert message.startswith("arbresampler:") and fragment in message, message
