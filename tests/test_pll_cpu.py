"""PLLBlock without a GPU: the speculate / verify / repair logic of luaradio_amd/csrc/pll_plan.h played on the CPU (tools/host_pll_check.hip), and
the self-checks of the f64 model the GPU tests compare against (tests/helpers/pll_model.py)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import pll_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pll_speculation_logic_on_the_cpu(tmp_path):
    """W against the pole radius, the serial / speculative plan, locked loops accepted everywhere and within 1e-6 of the serial loop, a short
    warm-up and a NaN ending in the repair walk: the functions the kernels call, driven by a host loop."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "host_pll_check")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "host_pll_check.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-4000:] + r.stderr[-2000:]


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
