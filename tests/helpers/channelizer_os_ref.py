"""Float64 reference of the K-channel analysis filterbank with frame hop D = K / R (PolyphaseChannelizerBlock, options["oversample"] = R),
written from its definition: K parallel chains FrequencyTranslator(-c/K) -> FIRFilter(h) -> Downsampler(D) with zero history, which is

    y_c[m] = exp(-j*2*pi*c*m*D/K) * sum_{i<M} h[i] * x[mD - i] * exp(+j*2*pi*c*i/K),   x[n] = 0 for n < 0,  frames m = 0, 1, ... while mD < len(x).

It is evaluated by polyphase folding in complex128, u_r[m] = sum_{i = r mod K} h[i] * x[mD - i], the rotation v[(r - mD) mod K] = u_r[m], then
y[m, :] = K * ifft(v).  Alongside, B[m] = sum_i |h[i]| * (|Re x[mD - i]| + |Im x[mD - i]|), the scale that bounds the rounding error of any
Float32 evaluation.  With D = K the rotation is the identity and every operation is that of channelizer_ref.channelize_f64."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from .channelizer_ref import U32, check_bars, error_ratio      # noqa: F401  (the bars are shared)


def nframes(n, D):
    return (n + D - 1) // D


def channelize_os_f64(x, h, K, R, block_elems=1 << 22):
    """(y complex128 [frames, K], B float64 [frames]) for the stream x (complex64), the prototype h (its Float32 values) and hop K / R"""
    assert K % R == 0
    D = K // R
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    M, n = len(h), len(x)
    F = nframes(n, D)
    y = np.empty((F, K), np.complex128)
    B = np.empty(F, np.float64)
    if F == 0:
        return y, B
    Mp = (M + K - 1) // K * K                      # window padded to whole polyphase rows: h[i] = 0 for M <= i < Mp
    hr = np.zeros(Mp)
    hr[:M] = h
    hr = hr[::-1].copy()                           # hr[j] multiplies window entry j = x[mD - (Mp - 1 - j)]
    ha = np.abs(hr)
    xp = np.concatenate([np.zeros(Mp - 1, np.complex64), x.astype(np.complex64, copy=False)])
    win = sliding_window_view(xp, Mp)[::D][:F]     # row m = x[mD - Mp + 1 .. mD], a view
    r = np.arange(K)
    rows = max(1, block_elems // Mp)
    rows = (rows + R - 1) // R * R                 # blocks start at a frame of class 0
    for a in range(0, F, rows):
        w = win[a:a + rows]
        p = w * hr                                  # complex128
        u = p[:, ::-1].reshape(len(w), Mp // K, K).sum(axis=1)       # column r = taps i = r mod K
        v = np.empty_like(u)
        for cls in range(R):                        # frames a + cls, a + cls + R, ...: m D mod K = cls D
            v[cls::R, (r - cls * D) % K] = u[cls::R]
        y[a:a + rows] = K * np.fft.ifft(v, axis=1)
        B[a:a + rows] = (np.abs(w.real) + np.abs(w.imag)) @ ha
    return y, B


def channelize_os_literal(x, h, K, R):
    """the defining sum term by term, O(frames * M * K): for small shapes only"""
    D = K // R
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    M, F = len(h), nframes(len(x), D)
    i = np.arange(M)
    y = np.zeros((F, K), np.complex128)
    for m in range(F):
        idx = m * D - i
        xs = np.where(idx >= 0, x[np.maximum(idx, 0)], 0)
        for c in range(K):
            y[m, c] = np.exp(-2j * np.pi * ((c * m * D) % K) / K) * np.sum(h * xs * np.exp(2j * np.pi * ((c * i) % K) / K))
    return y
