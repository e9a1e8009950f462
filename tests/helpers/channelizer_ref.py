"""Float64 reference of the K-channel analysis filterbank (PolyphaseChannelizerBlock), written from its definition and not from the
library's W matrix: K parallel chains FrequencyTranslator(-c/K) -> FIRFilter(h) -> Downsampler(K) with zero history, which is

    y_c[m] = sum_{i<M} h[i] * x[mK - i] * exp(+j*2*pi*c*i/K),      x[n] = 0 for n < 0,  frames m = 0, 1, ... while mK < len(x).

It is evaluated by polyphase folding in complex128, u_r[m] = sum_{i = r mod K} h[i] * x[mK - i], then y[m, :] = K * ifft(u[m, :]).
Alongside, B[m] = sum_i |h[i]| * (|Re x[mK - i]| + |Im x[mK - i]|), the scale that bounds the rounding error of any Float32 evaluation."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U32 = 2.0 ** -24          # unit roundoff of Float32


def nframes(n, K):
    return (n + K - 1) // K


def channelize_f64(x, h, K, block_elems=1 << 22):
    """(y complex128 [frames, K], B float64 [frames]) for the stream x (complex64) and the prototype h (its Float32 values)"""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    M, n = len(h), len(x)
    F = nframes(n, K)
    y = np.empty((F, K), np.complex128)
    B = np.empty(F, np.float64)
    if F == 0:
        return y, B
    Mp = (M + K - 1) // K * K                      # window padded to whole polyphase rows: h[i] = 0 for M <= i < Mp
    hr = np.zeros(Mp)
    hr[:M] = h
    hr = hr[::-1].copy()                           # hr[j] multiplies window entry j = x[mK - (Mp - 1 - j)]
    ha = np.abs(hr)
    xp = np.concatenate([np.zeros(Mp - 1, np.complex64), x.astype(np.complex64, copy=False)])
    win = sliding_window_view(xp, Mp)[::K][:F]     # row m = x[mK - Mp + 1 .. mK], a view
    rows = max(1, block_elems // Mp)
    for a in range(0, F, rows):
        w = win[a:a + rows]
        p = w * hr                                  # complex128
        u = p[:, ::-1].reshape(len(w), Mp // K, K).sum(axis=1)       # column r = taps i = r mod K
        y[a:a + rows] = K * np.fft.ifft(u, axis=1)
        B[a:a + rows] = (np.abs(w.real) + np.abs(w.imag)) @ ha
    return y, B


def channelize_literal(x, h, K):
    """the defining sum term by term, O(frames * M * K): for small shapes only"""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    M, F = len(h), nframes(len(x), K)
    i = np.arange(M)
    y = np.zeros((F, K), np.complex128)
    for m in range(F):
        idx = m * K - i
        xs = np.where(idx >= 0, x[np.maximum(idx, 0)], 0)
        for c in range(K):
            y[m, c] = np.sum(h * xs * np.exp(2j * np.pi * ((c * i) % K) / K))
    return y


def error_ratio(got, ref, B):
    """|got - ref| / (2^-24 * B[m]) per output; got is [frames, K]"""
    return np.abs(got.astype(np.complex128) - ref) / (U32 * B[:, None])


def check_bars(got, ref, B, M, agg):
    """per component |got - ref| <= (2M + 2) 2^-24 B[m] (worst case of a Float32 dot product of 2M terms with Float32-rounded
    weights), and rms(|got - ref| / (2^-24 B[m])) <= agg.  Returns the rms ratio; raises AssertionError with the worst frame."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(B > 0)
    lim = (2 * M + 2) * U32 * B[:, None]
    g = got.astype(np.complex128)
    bad = (np.abs(g.real - ref.real) > lim) | (np.abs(g.imag - ref.imag) > lim) | ~np.isfinite(g)
    if bad.any():
        m, c = np.argwhere(bad)[0]
        raise AssertionError("%d outputs over the per-output bar; first frame %d channel %d: got %r ref %r bar %.3g"
                             % (int(bad.sum()), m, c, got[m, c], ref[m, c], lim[m, 0]))
    r = float(np.sqrt(np.mean(error_ratio(got, ref, B) ** 2)))
    assert r <= agg, "aggregate error ratio %.4f > %.4f" % (r, agg)
    return r
