"""Restatements of the generator sources (luaradio_amd/csrc/kernels_source.h) in numpy, and the reference's literal SignalSource loop.

signal_closed_form(): sample n from turns(n) = p0 + n * step in wrapping uint64 arithmetic.  square / triangle / sawtooth / constant are
bit-equal to the device (exact double arithmetic, one double multiply, one double add, one rounding to Float32).  cosine / sine / exponential
restate the device's phasor polynomial (kernels_elem.h phasor_from_turns) in Float32 with every fused multiply-add done in double and rounded
once more - within one Float32 ulp of the device, not bit-equal; signal_exact() is the float64 closed form the device is held to.

signal_reference_loop(): radio/blocks/sources/signal.lua as written - a double phase accumulated sample by sample; exponential / cosine / sine
wrap it once per 8192-sample chunk and take the Float32 cos / sin of the phase rounded to Float32; the other waveforms wrap every sample.

philox_words() / uniform_random(): word j of the stream is output j & 3 of Philox4x32-10 on counter (lo32(j >> 2), hi32(j >> 2), 0, 0) and key
(lo32(seed), hi32(seed)); bit-equal to the device for all four sample types."""
import math

import numpy as np

TWO_PI = 6.283185307179586
CHUNK = 8192
MASK64 = (1 << 64) - 1
REAL_SIGNALS = ("cosine", "sine", "square", "triangle", "sawtooth", "constant")
SIGNALS = ("exponential",) + REAL_SIGNALS


def fx(x):
    """a fraction of a turn in 0.64 fixed point: uint64(rint(ldexp(x - floor(x), 64))) mod 2^64"""
    return int(np.rint(math.ldexp(x - math.floor(x), 64))) & MASK64


def turns(frequency, rate, phase, n0, count):
    """turns(n) for n in [n0, n0 + count) as uint64, wrapping"""
    step, p0 = fx(frequency / rate), fx(phase / TWO_PI)
    n = (np.arange(count, dtype=np.uint64) + np.uint64(n0 & MASK64))
    with np.errstate(over="ignore"):
        return np.uint64(p0) + n * np.uint64(step)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def phasor_from_turns(t):
    """kernels_elem.h phasor_from_turns on a uint64 array: (cos, sin) of 2 pi t / 2^64 as Float32 arrays"""
    f = np.float32
    with np.errstate(over="ignore"):
        t = t + np.uint64(1 << 61)
    q = (t >> np.uint64(62)).astype(np.int64)
    ri = (((t << np.uint64(2)) >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
    phi = ri.astype(f) * f(3.6572952e-10)
    z = phi * phi
    full = lambda v: np.full(z.shape, v, f)                                                                     # noqa: E731
    sp = _fma(_fma(_fma(full(-1.9515295891e-4), z, full(8.3321608736e-3)), z, full(-1.6666654611e-1)), z * phi, phi)
    cp = _fma(_fma(_fma(full(2.443315711809948e-5), z, full(-1.388731625493765e-3)), z, full(4.166664568298827e-2)), z * z,
              _fma(full(-0.5), z, full(1.0)))
    odd = (q & 1) == 1
    cs, sn = np.where(odd, -sp, cp), np.where(odd, cp, sp)
    neg = (q & 2) == 2
    return np.where(neg, -cs, cs).astype(f), np.where(neg, -sn, sn).astype(f)


def signal_closed_form(signal, frequency, rate, amplitude=1.0, phase=0.0, offset=0.0, n0=0, count=CHUNK):
    """samples [n0, n0 + count) of the device's SignalSource: complex64 for "exponential", float32 otherwise"""
    amplitude, offset = float(amplitude), float(offset)
    if signal == "constant":
        return np.full(count, np.float32(amplitude), np.float32)
    t = turns(frequency, rate, phase, n0, count)
    if signal in ("exponential", "cosine", "sine"):
        c, s = phasor_from_turns(t)
        if signal == "exponential":
            out = np.empty(count, np.complex64)
            out.real = (c.astype(np.float64) * amplitude).astype(np.float32)
            out.imag = (s.astype(np.float64) * amplitude).astype(np.float32)
            return out
        w = (c if signal == "cosine" else s).astype(np.float64)
    else:
        td = (t >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        first = t < np.uint64(1 << 63)
        if signal == "square":
            w = np.where(first, 1.0, -1.0)
        elif signal == "triangle":
            w = np.where(first, 1.0 - 4.0 * td, 4.0 * td - 3.0)
        elif signal == "sawtooth":
            w = 2.0 * td - 1.0
        else:
            raise ValueError('Unsupported signal ("%s")' % signal)
    return (w * amplitude + offset).astype(np.float32)


def signal_exact(signal, frequency, rate, amplitude=1.0, phase=0.0, offset=0.0, n0=0, count=CHUNK):
    """cosine / sine / exponential as the float64 closed form of the exact turns (complex128 for "exponential", float64 otherwise)"""
    t = turns(frequency, rate, phase, n0, count)
    hi, lo = (t >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, (t & np.uint64(2047)).astype(np.float64) * 2.0 ** -64
    a = 2.0 * np.pi * (hi + lo)
    if signal == "exponential":
        return amplitude * (np.cos(a) + 1j * np.sin(a))
    return amplitude * (np.cos(a) if signal == "cosine" else np.sin(a)) + offset


def signal_reference_loop(signal, frequency, rate, amplitude=1.0, phase=0.0, offset=0.0, count=CHUNK):
    """radio/blocks/sources/signal.lua, chunk after chunk of 8192 samples, the first `count` samples"""
    omega = 2 * math.pi * (frequency / rate)
    if signal == "constant":
        return np.full(count, np.float32(amplitude), np.float32)
    if signal in ("exponential", "cosine", "sine"):
        out = np.empty(count, np.complex64 if signal == "exponential" else np.float32)
        ph = float(phase)
        for at in range(0, count, CHUNK):
            # self.phase = self.phase + self.omega, 8192 times: a cumulative sum adds in the same order
            steps = np.full(CHUNK + 1, omega, np.float64)
            steps[0] = ph
            acc = np.cumsum(steps)
            p32 = acc[:CHUNK].astype(np.float32)
            c, s = np.cos(p32).astype(np.float64), np.sin(p32).astype(np.float64)          # ffi.C.cosf / sinf of the phase as a float
            m = min(CHUNK, count - at)
            if signal == "exponential":
                out.real[at:at + m] = (c * amplitude).astype(np.float32)[:m]
                out.imag[at:at + m] = (s * amplitude).astype(np.float32)[:m]
            else:
                out[at:at + m] = ((c if signal == "cosine" else s) * amplitude + offset).astype(np.float32)[:m]
            ph = float(acc[CHUNK])
            while ph > 2 * math.pi:
                ph -= 2 * math.pi
        return out
    pi, two_pi = math.pi, 2 * math.pi
    phi = float(phase)
    vals = np.empty(count, np.float64)
    for i in range(count):
        if signal == "square":
            vals[i] = (1.0 * amplitude + offset) if phi < pi else (-1.0 * amplitude + offset)
        elif signal == "triangle":
            vals[i] = ((1 - (2 / pi) * phi) * amplitude + offset) if phi < pi else ((-1 + (2 / pi) * (phi - pi)) * amplitude + offset)
        elif signal == "sawtooth":
            vals[i] = (-1 + (1 / pi) * phi) * amplitude + offset
        else:
            raise ValueError('Unsupported signal ("%s")' % signal)
        phi = phi + omega
        phi = (phi - two_pi) if phi >= two_pi else phi
    return vals.astype(np.float32)


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two; returns the four output words as uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & np.uint64(0xFFFFFFFF) for v in counter]
    k = [int(v) & 0xFFFFFFFF for v in key]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & m32]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return [v.astype(np.uint32) for v in c]


def philox_words(seed, j0, count):
    """words w(j), j in [j0, j0 + count) (indices modulo 2^64), as uint32"""
    with np.errstate(over="ignore"):
        j = np.arange(count, dtype=np.uint64) + np.uint64(j0 & MASK64)
    b = j >> np.uint64(2)
    first = int(b[0]) if count else 0
    nblocks = (int(b[-1]) - first + 1) if count else 0
    blocks = np.arange(nblocks, dtype=np.uint64) + np.uint64(first)
    out = philox4x32_10((blocks & np.uint64(0xFFFFFFFF), blocks >> np.uint64(32), 0 * blocks, 0 * blocks), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    table = np.stack(out, axis=1).reshape(-1)                   # word 4 (b - first) + r
    return table[(j - np.uint64(4 * first)).astype(np.int64)] if count else np.zeros(0, np.uint32)


def uniform_random(type_name, lo, hi, seed, n0, count):
    """samples [n0, n0 + count) of the device's UniformRandomSource: "cf32" complex64, "f32" float32, "byte" / "bit" uint8"""
    seed = int(seed)
    if type_name == "cf32":
        w = philox_words(seed, 2 * n0, 2 * count)
        v = (float(lo) + (float(hi) - float(lo)) * (w.astype(np.float64) * 2.0 ** -32)).astype(np.float32)
        return v.view(np.complex64)
    w = philox_words(seed, n0, count)
    if type_name == "f32":
        return (float(lo) + (float(hi) - float(lo)) * (w.astype(np.float64) * 2.0 ** -32)).astype(np.float32)
    if type_name == "byte":
        return (np.uint64(int(lo)) + ((w.astype(np.uint64) * np.uint64(int(hi) - int(lo) + 1)) >> np.uint64(32))).astype(np.uint8)
    if type_name == "bit":
        return (w >> np.uint32(31)).astype(np.uint8)
    raise ValueError("Unsupported data type")
