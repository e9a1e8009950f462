"""The contract of ArbitraryResamplerBlock (luaradio_amd/csrc/kernels_arbresample.h) in numpy and Python big integers.

Absolute output m sits at u = m * step in 16.48 fixed point of an input sample, step = rint(2^48 / ratio); i = u >> 48, f = u mod 2^48,
p = f >> (48 - log2 P), mu = ((f >> (24 - log2 P)) mod 2^24) * 2^-24.  y[m] = sum_k c_k x[i - k], c_k = G[p][k] + mu D[p][k], x[j] = 0 for j < 0.
model_f64 keeps the Float32 G, D and mu of the device and forms every product and sum in double."""
import math

import numpy as np

from luaradio_amd import filter_utils

FRAC = 48
ONE = 1 << FRAC


def step_of(ratio):
    return int(np.rint(2.0 ** FRAC / ratio))


def taps_per_phase(ratio, T0=16):
    return 2 * math.ceil(T0 / (2 * min(1.0, ratio)))


def tables_from_taps(h, P):
    """(G, D), each (P, T) Float32: G[p][k] = h[k P + p], row P = row 0 one tap later, D[p][k] = fl32(G[p + 1][k] - G[p][k])"""
    h = np.asarray(h, np.float32)
    assert len(h) % P == 0
    T = len(h) // P
    G = np.zeros((P + 1, T), np.float32)
    G[:P] = h.reshape(T, P).T
    G[P, :T - 1] = G[0, 1:]
    D = (G[1:] - G[:P]).astype(np.float32)
    assert D.dtype == np.float32 and (G[1:] - G[:P]).dtype == np.float32
    return np.ascontiguousarray(G[:P]), D


def prototype(ratio, P=64, T0=16):
    """the default design: P * firwin_lowpass(P T, min(1, ratio) / P) in double, rounded once to Float32"""
    T = taps_per_phase(ratio, T0)
    return (P * np.asarray(filter_utils.firwin_lowpass(P * T, min(1.0, ratio) / P), np.float64)).astype(np.float32)


def tables(ratio, P=64, T0=16):
    """(G, D, T, step) of the default design"""
    G, D = tables_from_taps(prototype(ratio, P, T0), P)
    return G, D, G.shape[1], step_of(ratio)


def position(m, step, log2p):
    """(i, p, mu24) of absolute output m, in Python integers"""
    u = m * step
    f = u & (ONE - 1)
    return u >> FRAC, f >> (FRAC - log2p), (f >> (24 - log2p)) & 0xFFFFFF


def positions(step, m0, count, log2p=6):
    """i (Python integers, a list), p (int64) and mu (Float32, exact) of outputs m0 .. m0 + count - 1"""
    pos = [position(m0 + j, step, log2p) for j in range(count)]
    i = [q[0] for q in pos]
    p = np.array([q[1] for q in pos], np.int64)
    mu = (np.array([q[2] for q in pos], np.float64) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(mu.astype(np.float64) * 2.0 ** 24, [q[2] for q in pos])
    return i, p, mu


def output_count(Q, step):
    """outputs that exist after Q inputs: the m with (m * step) >> 48 < Q"""
    return -((-Q << FRAC) // step)


def model_f64(x, G, D, step, m0=0, count=None, x0=0):
    """outputs m0 .. m0 + count - 1 of the stream whose sample x0 + j is x[j] and which is zero elsewhere (count None: every output whose newest
    input lies in front of x0 + len(x)).  Returns (y in double, sum_k |c_k| per output)."""
    P, T = G.shape
    log2p = P.bit_length() - 1
    assert 1 << log2p == P
    if count is None:
        count = output_count(x0 + len(x), step) - m0
    i, p, mu = positions(step, m0, count, log2p)
    x = np.asarray(x)
    xz = np.concatenate([np.zeros(T, x.dtype), x]).astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    rel = np.array([ii - x0 for ii in i], np.int64)                     # index of x[i] in x
    assert len(rel) == 0 or (rel.max() < len(x) and rel.min() >= -1)
    idx = rel[:, None] + T - np.arange(T)[None, :]                      # x[i - k] in xz, >= 0; in front of x: the T zeros
    c = G[p].astype(np.float64) + mu.astype(np.float64)[:, None] * D[p].astype(np.float64)
    return np.sum(c * xz[idx], axis=1), np.sum(np.abs(c), axis=1)
