"""The f64 restatement of radio/blocks/signal/pll.lua:113-167 the PLL tests compare against, with its Float32 roundings: the VCO sample is a
ComplexFloat32, x * conj(vco) is ComplexFloat32.__mul (a double expression stored as Float32 per component), and error is the Float32 of the
double atan2.  Plain Python floats are IEEE doubles, as Lua numbers are."""
import math

import numpy as np

TWO_PI = 2 * math.pi


def coefficients(loop_bandwidth, frequency_min, frequency_max, rate):
    """pll.lua:117-126 in its operation order: (alpha, beta, freq_min, freq_max)"""
    loop_bw = 2 * math.pi * (loop_bandwidth / rate)
    freq_min = 2 * math.pi * (frequency_min / rate)
    freq_max = 2 * math.pi * (frequency_max / rate)
    damping = math.sqrt(2) / 2
    loop_bw = loop_bw / (damping + 1 / (4 * damping))
    denom = (1 + 2 * damping * loop_bw + loop_bw * loop_bw)
    return (4 * damping * loop_bw) / denom, (4 * loop_bw * loop_bw) / denom, freq_min, freq_max


def initial_state(freq_min, freq_max):
    """(phi_locked, phi_multiplied, freq_locked), pll.lua:128-131"""
    return (0.0, 0.0, (freq_min + freq_max) / 2.0)


def advance(state, err, alpha, beta, freq_min, freq_max, multiplier):
    """the loop filter, clamp and wraps of one sample (pll.lua:151-163)"""
    pl, pm, fl = state
    fl = fl + beta * err
    pl = pl + fl + alpha * err
    pm = pm + fl * multiplier + alpha * err
    fl = freq_max if fl > freq_max else fl
    fl = freq_min if fl < freq_min else fl
    pl = pl - TWO_PI if pl > TWO_PI else pl
    pl = pl + TWO_PI if pl < -TWO_PI else pl
    pm = pm - TWO_PI if pm > TWO_PI else pm
    pm = pm + TWO_PI if pm < -TWO_PI else pm
    return (pl, pm, fl)


def run(x, loop_bandwidth, frequency_min, frequency_max, multiplier=1.0, rate=2.0, state=None):
    """PLLBlock:process(x): (out complex64, error float32, states float64 [n + 1, 3]); states[i] is the state BEFORE sample i."""
    alpha, beta, fmin, fmax = coefficients(loop_bandwidth, frequency_min, frequency_max, rate)
    s = initial_state(fmin, fmax) if state is None else tuple(state)
    x = np.asarray(x, dtype=np.complex64)
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)
    n = len(x)
    out = np.empty(n, dtype=np.complex128)
    err = np.empty(n, dtype=np.float32)
    states = np.empty((n + 1, 3), dtype=np.float64)
    f32 = np.float32
    for i in range(n):
        states[i] = s
        pl, pm, _ = s
        vr, vi = float(f32(math.cos(pl))), -float(f32(math.sin(pl)))
        out[i] = complex(math.cos(pm), math.sin(pm))
        re = float(f32(xr[i] * vr - xi[i] * vi))
        im = float(f32(xr[i] * vi + xi[i] * vr))
        e = f32(math.atan2(im, re)) if not (math.isnan(re) or math.isnan(im)) else f32(np.nan)
        err[i] = e
        s = advance(s, float(e), alpha, beta, fmin, fmax, multiplier)
    states[n] = s
    return out.astype(np.complex64), err, states


def replay(x, out, err, loop_bandwidth, frequency_min, frequency_max, multiplier=1.0, rate=2.0):
    """Replay consistency: the recurrence in f64 driven by the given error samples.  Returns (max |out[n] - cis(pm[n])|, max
    |error[n] - arg(x[n] conj(cis(pl[n])))| wrapped modulo 2 pi).  No sample is left out."""
    alpha, beta, fmin, fmax = coefficients(loop_bandwidth, frequency_min, frequency_max, rate)
    s = initial_state(fmin, fmax)
    x = np.asarray(x, dtype=np.complex64).astype(np.complex128)
    e64 = np.asarray(err, dtype=np.float64)
    n = len(x)
    pl, pm = np.empty(n), np.empty(n)
    for i in range(n):
        pl[i], pm[i] = s[0], s[1]
        s = advance(s, e64[i], alpha, beta, fmin, fmax, multiplier)
    ideal = np.exp(1j * pm)
    o = np.asarray(out).astype(np.complex128)
    d_out = float(np.max(np.abs(o - ideal))) if n else 0.0
    det = np.angle(x * np.exp(-1j * pl))
    d_err = float(np.max(np.abs(np.remainder(e64 - det + math.pi, TWO_PI) - math.pi))) if n else 0.0
    return d_out, d_err
