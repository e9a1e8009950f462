"""Float64 reference of the K-channel synthesis filterbank with frame hop D = K / R (PolyphaseSynthesizerBlock), written from its definition:
K parallel chains Upsampler(D) -> FIRFilter(g) -> FrequencyTranslator(+c / K) with zero history, summed, which is

    xhat[n] = sum_c exp(+j*2*pi*c*n/K) * sum_m g[n - m*D] * Y[m, c],     Y[m, :] = 0 for m < 0,   n = 0, 1, ... while floor(n / D) < frames.

synthesize_f64 evaluates it in its polyphase form in complex128, V[m, :] = K * ifft(Y[m, :]),
xhat[n] = sum_{q < Q, n mod D + q D < M} g[n mod D + q D] * V[floor(n / D) - q, n mod K], Q = ceil(M / D), and returns alongside
B[n] = sum_q |g[n mod D + q D]| * sum_c (|Re Y| + |Im Y|)[floor(n / D) - q, c], the scale of the rounding error of any Float32 evaluation.
synthesize_literal is the defining sum term by term; synthesize_f32_emulation the polyphase form in Float32 (V rounded to complex64, each
output one chain of fused multiply-adds, oldest frame first), whose own error ratio sets the aggregate bar of the device tests.

Error ratios rms(|err| / (2^-24 B[n])) over the shape matrix of tests/test_gpu_pfb_synthesizer.py (K x M in (K, K + 1, 3 K - 1, 16 K) x R in
(1, 2, 4), Hamming lowpass and random taps, random frames; 192 runs on one MI355X), emulation | device (the largest single ratio of the device):
    K = 8      0.106-0.282 | 0.106-0.280 (1.99)        K = 512    0.024-0.067 | 0.024-0.064 (0.31)
    K = 16     0.077-0.243 | 0.077-0.229 (1.21)        K = 1024   0.018-0.050 | 0.017-0.048 (0.21)
    K = 64     0.044-0.150 | 0.044-0.145 (0.79)        K = 2048   0.013-0.037 | 0.013-0.036 (0.17)
    K = 256    0.027-0.088 | 0.027-0.085 (0.45)        K = 4096   0.010-0.028 | 0.009-0.026 (0.12)
The device's ratio is 0.93-1.01 of the emulation's on the same inputs; B[n] sums over all K channels of a frame while the error of an output
grows like sqrt(K), which is why the ratios fall with K."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of Float32


def _geometry(Y, g, K, R):
    assert K % R == 0
    D = K // R
    Y = np.asarray(Y).reshape(-1, K)
    g = np.asarray(g, dtype=np.float32)
    M = len(g)
    Q = (M + D - 1) // D
    gp = np.zeros(Q * D, np.float32)
    gp[:M] = g
    live = np.zeros(Q * D, bool)
    live[:M] = True
    F = len(Y)
    f, d = np.arange(F)[:, None], np.arange(D)[None, :]
    cols = ((f % R) * D + d) % K                     # n mod K for n = f D + d
    return Y, gp.reshape(Q, D), live.reshape(Q, D), D, Q, F, cols


def _column_view(V, Q, q, cols):
    """V[f - q, cols[f, d]] with zero frames before the stream; V carries Q - 1 zero rows in front"""
    F = len(cols)
    rows = np.arange(F)[:, None] + (Q - 1 - q)
    return V[rows, cols]


def synthesize_f64(Y, g, K, R):
    """(xhat complex128 [frames * D], B float64 [frames * D]) for the frames Y (complex64 [frames, K] or flat) and the prototype g (its Float32
    values)"""
    Y, gq, live, D, Q, F, cols = _geometry(Y, g, K, R)
    V = np.concatenate([np.zeros((Q - 1, K), np.complex128), K * np.fft.ifft(Y.astype(np.complex128), axis=1)])
    Yc = Y.astype(np.complex128)
    S = np.concatenate([np.zeros(Q - 1), (np.abs(Yc.real) + np.abs(Yc.imag)).sum(axis=1)])
    x = np.zeros((F, D), np.complex128)
    B = np.zeros((F, D), np.float64)
    for q in range(Q - 1, -1, -1):
        w = np.where(live[q], gq[q].astype(np.float64), 0.0)
        x += w * np.where(live[q], _column_view(V, Q, q, cols), 0.0)
        B += np.abs(w) * S[np.arange(F) + (Q - 1 - q)][:, None]
    return x.reshape(-1), B.reshape(-1)


def synthesize_literal(Y, g, K, R):
    """the K chains term by term, O(frames * D * frames * K): for small shapes only"""
    D = K // R
    Y = np.asarray(Y).reshape(-1, K).astype(np.complex128)
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    M, F = len(g), len(Y)
    c = np.arange(K)
    x = np.zeros(F * D, np.complex128)
    for n in range(F * D):
        per_channel = np.zeros(K, np.complex128)
        for m in range(F):
            i = n - m * D
            if 0 <= i < M:
                per_channel += g[i] * Y[m]
        x[n] = np.sum(np.exp(2j * np.pi * ((c * n) % K) / K) * per_channel)
    return x


def _ifft_c64(Y, K):
    """K * ifft in single precision: numpy's own where it keeps complex64, else a radix-2 decimation in time in complex64"""
    Y = np.ascontiguousarray(Y, np.complex64)
    probe = np.fft.ifft(np.zeros(8, np.complex64))
    if probe.dtype == np.complex64:
        return (np.fft.ifft(Y, axis=1) * np.float32(K)).astype(np.complex64)
    bits = K.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(K)])
    a = Y[:, rev].copy()
    half = 1
    while half < K:
        w = np.exp(2j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        a = a.reshape(len(Y), -1, 2, half)
        t = (a[:, :, 1, :] * w).astype(np.complex64)
        a = np.stack([a[:, :, 0, :] + t, a[:, :, 0, :] - t], axis=2).astype(np.complex64).reshape(len(Y), K)
        half *= 2
    return a


def _fma32(a, b, c):
    """float32(a * b + c) for Float32 arrays: the product of two Float32 is exact in float64, so one float64 add and one rounding remain"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def synthesize_f32_emulation(Y, g, K, R):
    """the same algorithm in Float32: V = K * ifft(Y) in complex64, every output one fused multiply-add chain over q = Q - 1 ... 0 (oldest frame
    first) with the terms n mod D + q D >= M skipped.  Returns complex64 [frames * D]."""
    Y, gq, live, D, Q, F, cols = _geometry(Y, g, K, R)
    V = np.concatenate([np.zeros((Q - 1, K), np.complex64), _ifft_c64(Y, K)])
    re = np.zeros((F, D), np.float32)
    im = np.zeros((F, D), np.float32)
    for q in range(Q - 1, -1, -1):
        v = _column_view(V, Q, q, cols)
        w = np.broadcast_to(gq[q], (F, D))
        re = np.where(live[q], _fma32(w, v.real, re), re)
        im = np.where(live[q], _fma32(w, v.imag, im), im)
    return (re + 1j * im).astype(np.complex64).reshape(-1)


def error_ratio(got, ref, B):
    """|got - ref| / (2^-24 * B[n]) per output where B[n] > 0"""
    ok = B > 0
    return np.abs(np.asarray(got).astype(np.complex128) - ref)[ok] / (U32 * B[ok])


def rms_ratio(got, ref, B):
    return float(np.sqrt(np.mean(error_ratio(got, ref, B) ** 2)))


def check_bars(got, ref, B, K, Q, agg):
    """per component |got - ref| <= (2 K Q + 2) 2^-24 B[n] (the worst case of direct summation: a gross-error and non-finite catch), and
    rms(|got - ref| / (2^-24 B[n])) <= agg.  Returns the rms ratio; raises AssertionError with the first output over its bar."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    lim = (2 * K * Q + 2) * U32 * B
    g = got.astype(np.complex128)
    bad = (np.abs(g.real - ref.real) > lim) | (np.abs(g.imag - ref.imag) > lim) | ~np.isfinite(g)
    if bad.any():
        n = int(np.argmax(bad))
        raise AssertionError("%d outputs over the per-output bar; first n = %d: got %r ref %r bar %.3g" % (int(bad.sum()), n, got[n], ref[n], lim[n]))
    r = rms_ratio(got, ref, B)
    assert r <= agg, "aggregate error ratio %.4f > %.4f" % (r, agg)
    return r
