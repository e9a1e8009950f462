"""CPU models of BinaryPhaseCorrectorBlock (radio/blocks/signal/binaryphasecorrector.lua:43-73).

Three forms of the phase average after each measurement (absolute samples 0, I, 2I, ...):
  lua_average       the reference's loop literally: a double running sum that adds phi/N and subtracts the evicted value as the Float32
                    it was stored as (phi_state is a Float32 vector), so it drifts from the window mean as a random walk
  window_mean       the mean of the last N phases in double, the window starting as N zeros (the reference's spec generator,
                    tests/blocks/signal/binaryphasecorrector_spec.py)
  fixed_average     the device's form (luaradio_amd/csrc/kernels_phasecorr.h): phases quantised to int64 q = rint(phi 2^s), exact window sums,
                    avg = W / (N 2^s)
and rotate(), which applies an average per measurement to the samples as the reference does (rotation rounded to ComplexFloat32, the product
in double, each component rounded once).  A NaN phase makes every later average NaN."""
import math

import numpy as np

HALF_PI = math.pi / 2


def phases(x, I):
    """the clamped phase of every measured sample x[0], x[I], ... (binaryphasecorrector.lua:47-52), float64"""
    m = np.asarray(x, np.complex64)[::I]
    phi = np.arctan2(m.imag.astype(np.float64), m.real.astype(np.float64))
    phi = np.where(phi < -HALF_PI, phi + math.pi, phi)
    return np.where(phi > HALF_PI, phi - math.pi, phi)


def _sticky_nan(avg, phi):
    bad = np.flatnonzero(np.isnan(phi))
    if len(bad):
        avg = avg.copy()
        avg[bad[0]:] = np.nan
    return avg


def lua_average(phi, N):
    state = [0.0] * N                   # Float32 values, oldest first
    avg, out = 0.0, np.empty(len(phi))
    for k, p in enumerate(phi.tolist()):
        last = state.pop(0)
        state.append(float(np.float32(p)))
        avg = avg + p / N - last / N
        out[k] = avg
    return out


def window_mean(phi, N):
    """exact window sums (math.fsum) - for short runs"""
    padded = [0.0] * (N - 1) + phi.tolist()
    out = np.array([math.fsum(padded[k:k + N]) / N for k in range(len(phi))]) if not np.isnan(phi).any() else None
    if out is None:
        out = np.array([sum(padded[k:k + N]) / N for k in range(len(phi))])
    return _sticky_nan(out, phi)


def window_mean_fast(phi, N):
    """window sums as differences of a float64 prefix sum (error ~ 1e-16 of the prefix) - for long runs"""
    p = np.where(np.isnan(phi), 0.0, phi)
    c = np.concatenate([np.zeros(N), np.cumsum(p)])
    return _sticky_nan((c[N:] - c[:-N]) / N, phi)


def quant_shift(N):
    return min(52, 61 - math.ceil(math.log2(2 * N)))


def fixed_average(phi, N):
    s = quant_shift(N)
    q = np.rint(np.where(np.isnan(phi), 0.0, phi) * 2.0 ** s).astype(np.int64)
    with np.errstate(over="ignore"):
        c = np.concatenate([np.zeros(N, np.int64), np.cumsum(q, dtype=np.int64)])      # wraps like the device's unsigned sums
        w = c[N:] - c[:-N]
    return _sticky_nan(w.astype(np.float64) / (float(N) * 2.0 ** s), phi)


def rotate(x, avg, I, real=False):
    """y[i] = x[i] * ComplexFloat32(cos(-avg), sin(-avg)) of the last measurement at or before i"""
    x = np.asarray(x, np.complex64)
    a = np.repeat(avg, I)[:len(x)]
    cr, ci = np.cos(-a).astype(np.float32).astype(np.float64), np.sin(-a).astype(np.float32).astype(np.float64)
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)
    yr = (xr * cr - xi * ci).astype(np.float32)
    if real:
        return yr
    return (yr + 1j * (xr * ci + xi * cr).astype(np.float32)).astype(np.complex64)


def correct(x, N, I=32, form="fixed"):
    phi = phases(x, I)
    avg = {"lua": lua_average, "mean": window_mean, "mean_fast": window_mean_fast, "fixed": fixed_average}[form](phi, N)
    return rotate(x, avg, I)
