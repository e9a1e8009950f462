"""PLLBlock without a GPU: the speculate / verify / repair logic of luaradio_amd/csrc/pll_plan.h played on the CPU (tools/host_pll_check.hip), and
the self-checks of the f64 model the GPU tests compare against (tests/helpers/pll_model.py)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import pll_model as M
from tests.helpers import pll_signals as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6                             # the bar of tests/test_gpu_pll.py


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """tools/host_pll_check.hip, built once for this file"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("pll") / "host_pll_check")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "host_pll_check.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_pll_speculation_logic_on_the_cpu(tool):
    """W against the pole radius, the serial / speculative plan, locked loops accepted everywhere and within 1e-6 of the serial loop, a short
    warm-up and a NaN ending in the repair walk: the functions the kernels call, driven by a host loop."""
    r = subprocess.run([tool], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-4000:] + r.stderr[-2000:]


def play(tool, tmp_path, x, loop, mult, rate=2.0, segment=64):
    """one call of the plan over x (the tool's file mode): its counts and the largest out / error difference from its serial path per quarter"""
    path = str(tmp_path / "x.cf32")
    np.asarray(x, dtype=np.complex64).tofile(path)
    r = subprocess.run([tool, path] + [repr(float(v)) for v in (*loop, mult, rate)] + [str(segment)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head, out, error = r.stdout.strip().splitlines()
    words = head.split()
    got = {k: int(v) for k, v in zip(words[0::2], words[1::2])}
    assert out.split()[0] == "out" and error.split()[0] == "error"
    got["out"], got["error"] = [float(v) for v in out.split()[1:]], [float(v) for v in error.split()[1:]]
    assert got["n"] == len(x) and got["speculate"] == 1 and len(got["out"]) == 4 and len(got["error"]) == 4
    return got


def within_the_bar(what, got):
    print("%s: nseg %d rejected %d repaired %d, vs serial out %s error %s" % (what, got["nseg"], got["rejected"], got["repaired"],
                                                                              " ".join("%.2g" % v for v in got["out"]), " ".join("%.2g" % v for v in got["error"])))
    assert max(got["out"]) <= EPS and max(got["error"]) <= EPS


@pytest.mark.parametrize("name", ["burst", "gap", "early_and_late"])
def test_signals_that_are_repaired_in_part(tool, tmp_path, name):
    """The walk starts and stops inside the call: some segments rerun, most not.  gap: a segment behind a repaired one is accepted again from its
    speculated entry (fewer reruns than rejections).  early_and_late: segment 1 and the partial last segment are among the rerun ones."""
    got = play(tool, tmp_path, getattr(S, name)(), S.LOOP, 3.0)
    within_the_bar(name, got)
    assert got["nseg"] == (1025 if name == "early_and_late" else 1024)
    assert 0 < got["repaired"] < got["nseg"] - 1
    if name == "gap":
        assert got["repaired"] < got["rejected"]
    assert got["last_repaired"] == (1 if name == "early_and_late" else 0)
    if name == "early_and_late":
        # segment 1 alone, without the late burst: the first verified segment is rejected
        head = play(tool, tmp_path, S.early_and_late()[:8192], S.LOOP, 3.0)
        assert 0 < head["repaired"] < 40 and head["last_repaired"] == 0


@pytest.mark.parametrize("name, loop, mult, rate, segment", [
    ("jump", S.LOOP, 3.0, 2.0, 64),
    ("negative", S.NEGATIVE_LOOP, 3.0, 2.0, 64),
    ("locked", S.LOOP, -2.0, 2.0, 64),
    ("pilot", S.PILOT_LOOP, 2.0, S.PILOT_RATE, 0),
])
def test_signals_that_stay_speculated(tool, tmp_path, name, loop, mult, rate, segment):
    got = play(tool, tmp_path, getattr(S, name)(), loop, mult, rate, segment)
    within_the_bar("%s x%g" % (name, mult), got)
    assert got["rejected"] == 0 and got["repaired"] == 0 and got["nseg"] >= 512


def test_more_than_a_turn_per_sample(tool, tmp_path):
    """mult = 20 on the noisy carrier, 2^15 samples: nothing rejected, and phi_multiplied's residue (pll_plan.h: it grows with the stream) is still
    under the bar.  At 2^16 it is 7e-7 and rising, which no test asserts."""
    got = play(tool, tmp_path, S.locked()[:1 << 15], S.LOOP, 20.0)
    within_the_bar("locked x20, 2^15", got)
    assert got["rejected"] == 0
    more = play(tool, tmp_path, S.locked(), S.LOOP, 20.0)
    print("locked x20, 2^16: out %s" % " ".join("%.2g" % v for v in more["out"]))


@pytest.mark.parametrize("mult", [1.0, 3.0, -2.0])
@pytest.mark.parametrize("name", ["clean_centre", "clean_off"])
def test_clean_carriers_do_not_drift(tool, tmp_path, name, mult):
    """A carrier without noise: err is under PLL_LOCK_FLOOR, where speculated entries cannot be verified (every lane misses the long-running
    trajectory by the same amount and phi_multiplied integrates it: 3.4e-6 at mult 3, 4.8e-6 at mult -2 before the floor).  Every segment behind
    the pull-in (phase 0.3 shrinking by r = 0.959 per sample is under the floor after some 300 samples) is rerun serially, so both ports are
    the serial loop's."""
    got = play(tool, tmp_path, getattr(S, name)(), S.LOOP, mult)
    within_the_bar("%s x%g" % (name, mult), got)
    assert got["repaired"] >= got["nseg"] - 1 - 8


def test_model_coefficients_against_hand_computed_values():
    """PLLBlock(100, 18950, 19050, 2) at 220 500 Hz.  By hand: w0 = 2 pi 100 / 220500 = 2.849517e-3; d = 1 / sqrt 2; w = w0 / (d + 1 / (4 d)) =
    w0 / 1.0606602 = 2.686550e-3; denom = 1 + sqrt 2 w + w^2 = 1.0038066; alpha = 2 sqrt 2 w / denom = 7.569897e-3; beta = 4 w^2 / denom =
    2.876074e-5.  The block's own host arithmetic must be the model's, bit for bit."""
    alpha, beta, fmin, fmax = M.coefficients(100, 18950, 19050, 220500.0)
    assert abs(alpha - 7.569897e-3) < 5e-10
    assert abs(beta - 2.876074e-5) < 5e-12
    assert abs(fmin - 2 * math.pi * 18950 / 220500) < 1e-15 and abs(fmax - 2 * math.pi * 19050 / 220500) < 1e-15
    assert M.initial_state(fmin, fmax) == (0.0, 0.0, (fmin + fmax) / 2.0)
    from luaradio_amd.blocks import pll_coefficients
    assert pll_coefficients(100, 18950, 19050, 220500.0) == (alpha, beta, fmin, fmax)


def test_model_replays_its_own_output():
    """Replay consistency of the model itself, locked and on pure noise: out is cis(phi_multiplied) to Float32 rounding and error is the detector's
    answer to the Float32 spacing at pi (2.4e-7) - the check the GPU tests apply to the device where the loop is chaotic."""
    rng = np.random.default_rng(5)
    n = 1 << 13
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    locked = (np.exp(1j * (2 * np.pi * 0.1 * np.arange(n) + 0.3)) + 0.1 * noise).astype(np.complex64)
    for x in (locked, noise):
        out, err, states = M.run(x, 0.01, 0.19, 0.21, 3)
        assert states.shape == (n + 1, 3) and np.all(np.isfinite(states))
        d_out, d_err = M.replay(x, out, err, 0.01, 0.19, 0.21, 3)
        assert d_out <= 1e-7 and d_err <= 4e-7, (d_out, d_err)
    # in lock the error settles near zero and the oscillator runs at 3 x the carrier
    out, err, states = M.run(locked, 0.01, 0.19, 0.21, 3)
    assert abs(float(np.mean(err[n // 2:]))) < 0.01
    assert abs(states[-1, 2] - 2 * np.pi * 0.1) < 0.01
    # two calls carry the state: the same samples as one call
    a = M.run(locked[:1000], 0.01, 0.19, 0.21, 3)
    b = M.run(locked[1000:2000], 0.01, 0.19, 0.21, 3, state=a[2][-1])
    assert np.array_equal(np.concatenate([a[0], b[0]]), out[:2000]) and np.array_equal(np.concatenate([a[1], b[1]]), err[:2000])
