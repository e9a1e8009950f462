"""PLLBlock on the MI355X against the f64 model of pll.lua (tests/helpers/pll_model.py): the speculative path in lock (no repair, Chain.last_launches
= 4), the repair walk (5), the serial path (1), replay consistency where the loop is chaotic or sits on its clamp, the edges of the segment grid,
reset, NaN, refused parameters and time partitions, the streams of tests/helpers/pll_signals.py that are repaired in part, run a negative loop or
multiplier, or carry no noise, and the two receivers that wait on the PLL against the same topology built from the oracle."""
import functools
import math

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from luaradio_amd import blocks as B
from tests.helpers import pll_model as M
from tests.helpers import pll_signals as S

pytestmark = pytest.mark.gpu

N = 1 << 16
LOOP = (0.01, 0.19, 0.21)              # loop bandwidth, frequency_min, frequency_max at the jig's rate 2.0
EPS = 1e-6                             # the reference jig's epsilon
SPECULATED, REPAIRED, SERIAL = 4, 5, 1   # kernels a call launches on each path (stage_pll.h)
CUTS = (0, 1, 2, 3, 4, 104, 5000, 5001, 30000, 30001, 30002, N)      # one-sample calls, a call shorter than W = 541, long ones


def port(name, mult=3.0, knobs="", loop=LOOP, rate=2.0):
    blk = B.PLLOutBlock(*loop, mult, name)
    blk.rate = rate
    blk.op_knobs = knobs
    blk.differentiate([types.ComplexFloat32])
    blk.initialize()
    return blk


def cnoise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def locked_signal():
    x = (np.exp(1j * (2 * np.pi * 0.1 * np.arange(N) + 0.3)) + 0.1 * cnoise(N, 11)).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def locked_model(mult):
    out, err, states = M.run(locked_signal(), *LOOP, mult)
    for a in (out, err, states):
        a.setflags(write=False)
    return out, err, states


def ragged(chain, x, cuts=CUTS):
    return np.concatenate([chain.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])


def err_of(got, want):
    return float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))) if len(want) else 0.0


@pytest.mark.parametrize("mult", [3.0, 1 / 16])
def test_locked_parity_whole_and_ragged(mult):
    x = locked_signal()
    want = dict(zip(("out", "error"), locked_model(mult)[:2]))
    for name in ("out", "error"):
        ch = lr.Chain([port(name, mult, ":segment=64")])
        whole = ch.process(x)
        launches = ch.last_launches
        cut = ragged(lr.Chain([port(name, mult, ":segment=64")]), x)
        print("mult %g %s: whole %.3g ragged %.3g (launches %d)" % (mult, name, err_of(whole, want[name]), err_of(cut, want[name]), launches))
        assert launches == SPECULATED            # 1024 segments speculated, none repaired
        assert err_of(whole, want[name]) <= EPS
        assert err_of(cut, want[name]) <= EPS
    if mult == 3.0:
        # long enough for phi_multiplied to wrap many times
        pm = locked_model(mult)[2][:, 1]
        assert int(np.sum(np.diff(pm) < -math.pi)) > 10000


def test_block_returns_both_ports():
    x = locked_signal()[:8192]
    blk = lr.PLLBlock(*LOOP, 3)
    blk.rate = 2.0
    blk.differentiate([types.ComplexFloat32])
    blk.initialize()
    out, error = blk.process(x)
    assert out.dtype == np.complex64 and error.dtype == np.float32
    assert err_of(out, locked_model(3.0)[0][:8192]) <= EPS and err_of(error, locked_model(3.0)[1][:8192]) <= EPS
    assert [p.name for p in blk.signature[1]] == ["out", "error"]


def test_short_warmup_is_repaired():
    x = locked_signal()
    for name, want in zip(("out", "error"), locked_model(3.0)[:2]):
        ch = lr.Chain([port(name, 3.0, ":segment=64:warmup=8")])
        got = ch.process(x)
        assert ch.last_launches == REPAIRED
        print("warmup=8 %s: %.3g" % (name, err_of(got, want)))
        assert err_of(got, want) <= EPS


def test_serial_path():
    x = locked_signal()
    for name, want in zip(("out", "error"), locked_model(3.0)[:2]):
        ch = lr.Chain([port(name, 3.0, ":speculate=0")])
        got = ch.process(x)
        assert ch.last_launches == SERIAL
        default = lr.Chain([port(name, 3.0)]).process(x)
        print("serial %s: vs model %.3g, vs default path %.3g" % (name, err_of(got, want), err_of(got, default)))
        assert err_of(got, want) <= EPS
        assert err_of(got, default) <= EPS


def replay_check(x, mult=3.0, knobs="", cuts=None):
    run = (lambda ch: ch.process(x)) if cuts is None else (lambda ch: ragged(ch, x, cuts))
    out, error = run(lr.Chain([port("out", mult, knobs)])), run(lr.Chain([port("error", mult, knobs)]))
    d_out, d_err = M.replay(x, out, error, *LOOP, mult)
    print("replay: out %.3g error %.3g" % (d_out, d_err))
    assert d_out <= EPS and d_err <= EPS


def test_unlocked_input_is_replay_consistent():
    """pure noise: the loop is chaotic, so the device's own error samples drive an f64 replay (the model's own output passes at 2.4e-7)"""
    x = cnoise(N, 12)
    replay_check(x)
    replay_check(x, cuts=CUTS)


def test_carrier_outside_the_clamp_range():
    """freq_locked sits on the clamp (a 0.25 carrier with limits 0.19 .. 0.21)"""
    x = (np.exp(1j * 2 * np.pi * 0.125 * np.arange(N)) + 0.05 * cnoise(N, 13)).astype(np.complex64)
    states = M.run(x[:4096], *LOOP, 3.0)[2]
    assert np.mean(states[2048:, 2] == 2 * math.pi * (0.21 / 2.0)) > 0.5
    replay_check(x)
    replay_check(x, knobs=":segment=64")


@pytest.mark.parametrize("n", [0, 1, 63, 65, 4097])
def test_segment_grid_edges(n):
    """n = 0, 1, C - 1, C + 1 (serial by the plan), and 64 whole segments plus one sample (speculated)"""
    x = locked_signal()[:n]
    for name, want in zip(("out", "error"), locked_model(3.0)[:2]):
        ch = lr.Chain([port(name, 3.0, ":segment=64")])
        got = ch.process(x)
        assert len(got) == n and err_of(got, want[:n]) <= EPS
        if n == 4097:
            assert ch.last_launches == SPECULATED


def test_reset_restores_the_initial_state():
    x = locked_signal()[:20000]
    for name in ("out", "error"):
        blk = port(name, 3.0, ":segment=64")
        first = blk.process(x)
        moved = blk.process(x)
        blk.reset()
        again = blk.process(x)
        assert np.array_equal(first.view(np.uint8), again.view(np.uint8)) and not np.array_equal(first.view(np.uint8), moved.view(np.uint8))


def test_nan_sample():
    k = 20000
    x = locked_signal().copy()
    x[k] = complex(np.nan, 0.0)
    for name in ("out", "error"):
        clean = lr.Chain([port(name, 3.0, ":segment=64")]).process(locked_signal())
        got = lr.Chain([port(name, 3.0, ":segment=64")]).process(x)          # the call returns
        assert np.array_equal(got[:k].view(np.uint8), clean[:k].view(np.uint8))
        assert np.all(np.isnan(got[k + 1:].view(np.float32)))
        if name == "error":
            assert np.isnan(got[k])


@pytest.mark.parametrize("op, text", [
    ("pll:beta=1e-3:fmin=0.5:fmax=0.6", "missing parameter \"alpha\""),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5", "missing parameter \"fmax\""),
    ("pll:alpha=nan:beta=1e-3:fmin=0.5:fmax=0.6", "alpha must be finite"),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5:fmax=inf", "fmax must be finite"),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5:fmax=0.6:mult=inf", "mult must be finite"),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5:fmax=0.6:bandwidth=3", "unknown parameter \"bandwidth\""),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5:fmax=0.6:port=both", "port must be"),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5:fmax=0.6:segment=0", "segment must be"),
    ("pll:alpha=0.05:beta=1e-3:fmin=0.5:fmax=0.6:speculate=2", "speculate must be"),
])
def test_bad_parameters_are_refused(op, text):
    lr.init(0)
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 1)
    assert text in _lib.last_error()
    with pytest.raises(AssertionError):
        lr.PLLBlock(100, 18950)            # pll.lua:31: Missing argument #3


def test_time_partitions_are_refused():
    ch = lr.Chain([port("out")])
    with pytest.raises(lr.LrhipError, match="unbounded memory"):
        ch.halo()
    with pytest.raises(lr.LrhipError):
        ch.start_at(100000)


# ---- the streams of tests/helpers/pll_signals.py: tests/test_pll_cpu.py asserts on the CPU that each takes the path it was built for -------------
PARTIAL_CUTS = (0, 1, 30500, 30501, 31990, 40000)      # a boundary inside the burst, state carried out of a repaired run, serial calls in between
SIGNAL_LOOPS = {"negative": (S.NEGATIVE_LOOP, 2.0), "pilot": (S.PILOT_LOOP, S.PILOT_RATE)}


@functools.lru_cache(maxsize=None)
def signal_model(name, mult, n=None):
    loop, rate = SIGNAL_LOOPS.get(name, (S.LOOP, 2.0))
    out, err, states = M.run(getattr(S, name)()[:n], *loop, mult, rate=rate)
    for a in (out, err, states):
        a.setflags(write=False)
    return out, err, states


def compare(what, got, want):
    """prints the largest difference and, where it is over the bar, the first sample over it; then asserts the bar"""
    d = np.abs(got.astype(np.complex128) - want.astype(np.complex128))
    worst = float(d.max()) if len(d) else 0.0
    over = np.flatnonzero(d > EPS)
    print("%s: %.3g%s" % (what, worst, "" if not len(over) else " (first over the bar: sample %d, got %r, model %r; last: %d; %d in all)" % (
        over[0], got[over[0]], want[over[0]], over[-1], len(over))))
    assert len(got) == len(want) and worst <= EPS


def both_ports(name, mult, knobs="", n=None, launches=None, cuts=None):
    loop, rate = SIGNAL_LOOPS.get(name, (S.LOOP, 2.0))
    x = getattr(S, name)()[:n]
    got = {}
    for pname, want in zip(("out", "error"), signal_model(name, mult, n)[:2]):
        ch = lr.Chain([port(pname, mult, knobs, loop, rate)])
        got[pname] = ch.process(x) if cuts is None else ragged(ch, x, tuple(cuts) + (len(x),))
        if launches is not None:
            assert ch.last_launches == launches, (pname, ch.last_launches)
        compare("%s x%g %s%s %s" % (name, mult, knobs or "default plan", "" if cuts is None else " ragged", pname), got[pname], want)
    return got


@pytest.mark.parametrize("name", ["burst", "gap", "early_and_late"])
def test_partial_repair(name):
    """Lock lost and regained inside one call: the walk starts in mid-stream, stops, and the segments behind it stay speculated (CPU: 32, 35 and 18
    of 1024 segments rerun; in `gap` one is re-accepted from its speculated entry behind a repaired one; in `early_and_late` segment 1 and the
    37-sample last segment are rerun).  Then in calls cut inside the burst."""
    both_ports(name, 3.0, ":segment=64", launches=REPAIRED)
    both_ports(name, 3.0, "", launches=REPAIRED)
    got = both_ports(name, 3.0, ":segment=64", cuts=PARTIAL_CUTS)
    if name == "gap":
        # exact zeros: x * conj(vco) is (+-0, +-0), and atan2(+0, -0) = pi where the VCO sample has a negative real and a non-negative imaginary
        # part of its conjugate.  The model meets the case, and the device answers it the same way, sample for sample.
        pi32, want = np.float32(math.pi), signal_model(name, 3.0)[1]
        inside = slice(*S.BURST)
        assert int(np.sum(want[inside] == pi32)) > 0 and not np.any(want[inside] == -pi32)
        assert set(np.unique(want[inside]).tolist()) <= {0.0, float(pi32)}
        assert np.array_equal(got["error"][inside] == pi32, want[inside] == pi32)


def test_phase_jump_stays_speculated():
    """a 2 rad step of the carrier's phase: a transient that every lane sees with the same history, so nothing is rejected"""
    err = signal_model("jump", 3.0)[1]
    assert float(np.max(np.abs(err[40003:40010]))) > 1.5 and float(np.max(np.abs(err[39000:40003]))) < 0.6       # the step is there
    both_ports("jump", 3.0, ":segment=64", launches=SPECULATED)
    both_ports("jump", 3.0, "", launches=SPECULATED)


def test_negative_loop_and_negative_multiplier():
    """the < -2 pi wrap branches of pll_step: phi_locked running downward (a loop over -0.21 .. -0.19), and phi_multiplied running downward while
    phi_locked runs upward (mult = -2)"""
    states = signal_model("negative", 3.0)[2]
    assert int(np.sum(np.diff(states[:, 0]) > math.pi)) > 1000 and int(np.sum(np.diff(states[:, 0]) < -math.pi)) == 0
    assert int(np.sum(np.diff(states[:, 1]) > math.pi)) > 1000
    both_ports("negative", 3.0, ":segment=64", launches=SPECULATED)
    both_ports("negative", 3.0, ":segment=64", cuts=CUTS[:-1])
    states = signal_model("locked", -2.0)[2]
    assert int(np.sum(np.diff(states[:, 0]) < -math.pi)) > 1000 and int(np.sum(np.diff(states[:, 1]) > math.pi)) > 1000
    both_ports("locked", -2.0, ":segment=64", launches=SPECULATED)
    both_ports("locked", -2.0, ":segment=64", cuts=CUTS[:-1])


def test_more_than_a_turn_per_sample():
    """mult = 20: phi_multiplied gains 12.6 rad per sample, the single conditional wrap takes off 6.28, and the value grows without bound (the
    reference's behaviour).  2^15 samples: phi_multiplied's distance from the serial loop grows with the stream (pll_plan.h; on the CPU 4e-7 here,
    7.8e-7 at 2^16 and rising), so this is the longest stream the bar is asserted on."""
    n = 1 << 15
    assert float(signal_model("locked", 20.0, n)[2][-1, 1]) > 1e5
    both_ports("locked", 20.0, ":segment=64", n=n, launches=SPECULATED)
    both_ports("locked", 20.0, ":segment=64", n=n, cuts=[c for c in CUTS if c < n])


def test_the_receivers_pilot_loop():
    """PLLBlock(100, 18950, 19050, 2) at 220 500 Hz, W = 5 957: a whole call of 2^16 speculates (W + 2 C <= n / 2); ragged, the calls shorter than
    2 (W + 2 C) run serially in between"""
    both_ports("pilot", 2.0, "", launches=SPECULATED)
    both_ports("pilot", 2.0, "", cuts=CUTS[:-1])


@pytest.mark.parametrize("mult", [1.0, 3.0, -2.0])
@pytest.mark.parametrize("name", ["clean_centre", "clean_off"])
def test_clean_carriers_do_not_drift(name, mult):
    """No noise: the mean |err| is under PLL_LOCK_FLOOR, the segments are rerun serially, and phi_multiplied does not drift away from the model
    (before the floor, on the CPU: 3.4e-6 at mult 3 and 4.8e-6 at mult -2 on clean_centre, linear in time, with nothing rejected)."""
    both_ports(name, mult, ":segment=64", launches=REPAIRED)


def test_reset_after_a_repaired_call():
    x = S.burst()
    for name in ("out", "error"):
        blk = port(name, 3.0, ":segment=64")
        first = blk.process(x)
        blk.reset()
        again = blk.process(x)
        assert np.array_equal(first.view(np.uint8), again.view(np.uint8))
        compare("burst after reset %s" % name, again, signal_model("burst", 3.0)[0 if name == "out" else 1])


# ---- the receivers that waited on the PLL, against the same topology from the oracle's block functions and the PLL model ------------------------
FS = 1102500.0
RF_N = 1 << 20


class _Delay:
    """DelayBlock / the real part of HilbertTransformBlock: num_samples zeros in front"""

    def __init__(self, num_samples):
        self.k = num_samples

    def process(self, x):
        return np.concatenate([np.zeros(self.k, x.dtype), x[:len(x) - self.k]])


def _highpass_taps(cutoff, rate):
    """singlepolehighpassfilter.lua:34-45 in double, rounded to Float32 like the reference's tap vectors"""
    tau = 1 / (2 * math.pi * cutoff)
    tau = 1 / (2 * rate * math.tan(1 / (2 * rate * tau)))
    k = 2 * tau * rate
    return np.array([k / (1 + k), -k / (1 + k)], np.float32), np.array([1, (1 - k) / (1 + k)], np.float32)


def _complex_bandpass(cutoffs, rate):
    from oracle import oracle as O
    taps = types.ComplexFloat32.vector_from_array(lr.filter_utils.firwin_complex_bandpass(129, [c / (rate / 2) for c in cutoffs]))
    return O.FIR(taps, True)


def _check_audio(got, want, what):
    """the tolerance tests/test_gpu_rx.py applies to the mono receiver: RMS error <= 1e-5, largest < 1e-6"""
    assert len(got) == len(want)
    err = got.astype(np.float64) - want
    rms, worst = float(np.sqrt(np.mean(err ** 2))), float(np.max(np.abs(err)))
    print("%s: rms error %.3g, largest %.3g, signal rms %.3g" % (what, rms, worst, float(np.sqrt(np.mean(want.astype(np.float64) ** 2)))))
    assert rms <= 1e-5 and worst < 1e-6


def _separation_db(left, right, rate, tone=1e3):
    """power of the tone in the left output over the right one, after the filters have settled"""
    k = len(left) // 4
    t = np.arange(len(left) - k) / rate
    probe = np.exp(-2j * np.pi * tone * t) * np.hanning(len(t))
    return 20 * math.log10(abs(np.dot(left[k:].astype(np.float64), probe)) / abs(np.dot(right[k:].astype(np.float64), probe)))


def test_wbfm_stereo_receiver_against_the_oracle_topology():
    from oracle import oracle as O
    rng = np.random.default_rng(21)
    t = np.arange(RF_N) / FS
    left, right = np.sin(2 * np.pi * 1e3 * t), np.zeros(RF_N)            # a left-only 1 kHz tone
    # the subcarrier's phase against the pilot is the one this topology demodulates (its Delay(129) against the pilot filter's 64 samples)
    mpx = 0.45 * (left + right) + 0.1 * np.sin(2 * np.pi * 19e3 * t) + 0.45 * (left - right) * np.cos(2 * np.pi * 38e3 * t)
    x = np.exp(1j * (2 * np.pi * 250e3 * t + 2 * np.pi * 75e3 / FS * np.cumsum(mpx)))
    x = (x + 0.001 * (rng.standard_normal(RF_N) + 1j * rng.standard_normal(RF_N))).astype(np.complex64)
    got = lr.wbfm_stereo_receiver(FS, -250e3).process(**{"in": x})
    assert sorted(got) == ["left", "right"]

    r1 = FS / 5
    demod = O.FMDiscriminator(1.25).process(O.tuner(-250e3, 200e3, 5, FS, mode=O.MODE_LUA, rot_mode=O.MODE_F64).process(x))
    taps = types.Float32.vector_from_array(lr.filter_utils.fir_hilbert_transform(129, "hamming"))
    hilbert = (_Delay(64).process(demod) + 1j * O.FIR(taps, False).process(demod)).astype(np.complex64)
    delayed = _Delay(129).process(hilbert)
    pilot = _complex_bandpass([18e3, 20e3], r1).process(hilbert)
    pll_out = M.run(pilot, 100, 19e3 - 50, 19e3 + 50, 2, rate=r1)[0]
    lpr = np.ascontiguousarray(O.lowpass(128, 15e3, r1, True).process(delayed).real)
    lmr = np.ascontiguousarray(O.lowpass(128, 15e3, r1, True).process(O.multiply_conjugate(delayed, pll_out)).real)
    want = {}
    for name, mix in (("left", lpr + lmr), ("right", lpr - lmr)):
        b, a = O.fm_deemphasis_taps(75e-6, r1)
        want[name] = O.Downsampler(5, False).process(O.IIR(b, a, False).process(mix.astype(np.float32)))
    for name in ("left", "right"):
        _check_audio(got[name], want[name], name)
    sep_model, sep_device = _separation_db(want["left"], want["right"], r1 / 5), _separation_db(got["left"], got["right"], r1 / 5)
    print("separation: model %.2f dB, device %.2f dB" % (sep_model, sep_device))
    assert sep_model > 20.0                       # the input is stereo: the model itself separates it
    assert abs(sep_device - sep_model) <= 1.0


def test_am_synchronous_receiver_against_the_oracle_topology():
    from oracle import oracle as O
    rng = np.random.default_rng(22)
    ifreq, bw = 50e3, 5e3
    t = np.arange(RF_N) / FS
    x = 0.5 * (1 + 0.5 * np.sin(2 * np.pi * 440 * t)) * np.exp(2j * np.pi * (ifreq + 20) * t)          # 50 % depth, 20 Hz off the IF
    x = (x + 0.001 * (rng.standard_normal(RF_N) + 1j * rng.standard_normal(RF_N))).astype(np.complex64)
    got = lr.am_synchronous_receiver(FS, ifreq, bw).process(**{"in": x})
    assert list(got) == ["AGCBlock"]

    r1 = FS / 5
    filtered = _complex_bandpass([ifreq - bw, ifreq + bw], r1).process(O.decimator(5, FS, True).process(x))
    pll_out = M.run(filtered, 1000, ifreq - 100, ifreq + 100, 1.0, rate=r1)[0]
    audio = np.ascontiguousarray(O.multiply_conjugate(filtered, pll_out).real)
    b, a = _highpass_taps(100, r1)
    audio = O.Downsampler(10, False).process(O.lowpass(128, bw, r1, False).process(O.IIR(b, a, False).process(audio)))
    want = O.AGC("slow", -35, -75, r1 / 10, False).process(audio)
    _check_audio(got["AGCBlock"], want, "am synchronous")
