"""Python models of ZeroCrossingClockRecoveryBlock, SamplerBlock, SlicerBlock and DifferentialDecoderBlock, written from their documented
semantics (include/lrhip.h, luaradio_amd/csrc/kernels_digital.h): the literal per-sample loops, and the clock recovery's closed form with the
conditions under which it equals the loop."""
import math

import numpy as np


class ZcLiteral:
    """the reference loop: hysteresis, offset (a double) reset to P/2 at every flip, - 1 per sample, pulse + P below 1"""

    def __init__(self, P, T=0.0):
        self.P, self.T, self.h, self.o = float(P), float(T), False, float(P)

    def process(self, x):
        out = np.empty(len(x), np.float32)
        P, T, h, o = self.P, self.T, self.h, self.o
        for i, v in enumerate(x.tolist()):
            if not h and v > T:
                h, o = True, P / 2
            elif h and v < T:
                h, o = False, P / 2
            o = o - 1
            if o < 1:
                out[i] = 1
                o = o + P
            else:
                out[i] = -1
        self.h, self.o = h, o
        return out


def zc_closed_params(P):
    """(U, Pi, ks[2], c0[2]) of the closed form, or None where it is not proven (the conditions of stage_digital.h zc_prepare)"""
    P = float(P)
    if not (2.0 <= P < 2.0 ** 40):
        return None
    e = math.frexp(P)[1] - 1
    if P + 1.0 > 2.0 ** (e + 1):
        return None
    u = 2.0 ** (e - 52)
    U, Pi = 2 ** (52 - e), int(P / u)
    ks, c0 = [], []
    for o in (P, P / 2):
        k = 0
        while o >= 2.0:
            s = math.floor(o) - 1.0
            o -= s
            k += int(s)
        o = o - 1.0
        o1 = o + P
        if not (o >= 0.0 and o1 < P + 1.0):
            return None
        A = int(o1 / u)
        if A * u != o1 or not (0 <= A - Pi < U):
            return None
        ks.append(k)
        c0.append(((1 - k) * U - (A - Pi) - 1) % Pi)
    return U, Pi, ks, c0


def zc_pulses_closed(kind, k, params):
    """pulse (bool array) at k samples after a reset of `kind` (0 stream start, 1 crossing), closed form; k int64 array"""
    U, Pi, ks, c0 = params
    k = np.asarray(k, np.int64)
    kind = np.broadcast_to(np.asarray(kind), k.shape)
    # W = (c0 + k U) mod Pi, U = 2^s, in uint64 by doubling (every value < 2^54)
    r = (k.astype(np.uint64) % np.uint64(Pi))
    for _ in range(U.bit_length() - 1):
        r = (r * np.uint64(2)) % np.uint64(Pi)
    c = np.where(kind == 1, np.uint64(c0[1]), np.uint64(c0[0]))
    W = (r + c) % np.uint64(Pi)
    kss = np.where(kind == 1, ks[1], ks[0])
    return (k >= kss) & (W < np.uint64(U))


class ZcFast:
    """the same block, vectorised: last reset by a max-scan, F_kind(k) by the closed form (P where it holds) or the literal loop per reset"""

    def __init__(self, P, T=0.0):
        self.P, self.T = float(P), float(T)
        self.params = zc_closed_params(P)
        self.h, self.k, self.kind = -1, 0, 0            # hysteresis, samples since the reset, kind of reset

    def _F(self, kind, k):
        if self.params is not None:
            return zc_pulses_closed(kind, k, self.params)
        out = np.empty(len(k), bool)
        for i, (kd, kk) in enumerate(zip(np.asarray(kind).tolist(), np.asarray(k).tolist())):
            out[i] = _literal_pulse(self.P, kd, kk)
        return out

    def pulses(self, x):
        if self.params is None:                         # no closed form: the literal loop carries the state itself
            if not hasattr(self, "_lit"):
                self._lit = ZcLiteral(self.P, self.T)
            return self._lit.process(x) > 0
        n = len(x)
        xd = x.astype(np.float64)
        d = np.where(xd > self.T, 1, np.where(xd < self.T, -1, 0)).astype(np.int8)
        idx = np.arange(n)
        last_dec = np.maximum.accumulate(np.where(d != 0, idx, -1))
        prev_state = np.empty(n, np.int8)
        hist = np.where(last_dec >= 0, d[np.maximum(last_dec, 0)], self.h).astype(np.int8)
        prev_state[0] = self.h
        prev_state[1:] = hist[:-1]
        cross = (d != 0) & (d != prev_state)
        rpos = np.maximum.accumulate(np.where(cross, idx, -1))
        kind = np.where(rpos >= 0, 1, self.kind)
        k = np.where(rpos >= 0, idx - rpos, idx + self.k).astype(np.int64)
        p = self._F(kind, k)
        if n:
            self.h = int(hist[-1])
            self.kind, self.k = int(kind[-1]), int(k[-1]) + 1
        return p

    def process(self, x):
        return np.where(self.pulses(x), 1, -1).astype(np.float32)


def _literal_pulse(P, kind, k):
    o = P if kind == 0 else P / 2
    pulse = False
    for _ in range(k + 1):
        o = o - 1
        pulse = o < 1
        if pulse:
            o = o + P
    return pulse


class SamplerModel:
    def __init__(self):
        self.high = False

    def process(self, data, clock):
        keep = []
        for i, c in enumerate(clock.tolist()):
            if not self.high and c > 0:
                keep.append(i)
                self.high = True
            elif self.high and c < 0:
                self.high = False
        return data[np.array(keep, np.int64)]


class SamplerFast:
    """vectorised SamplerModel"""

    def __init__(self):
        self.h = -1

    def process(self, data, clock):
        n = len(clock)
        d = np.where(clock > 0, 1, np.where(clock < 0, -1, 0)).astype(np.int8)
        idx = np.arange(n)
        last_dec = np.maximum.accumulate(np.where(d != 0, idx, -1))
        hist = np.where(last_dec >= 0, d[np.maximum(last_dec, 0)], self.h)
        prev = np.concatenate([[self.h], hist[:-1]]) if n else hist
        emit = (d > 0) & (prev < 0)
        if n:
            self.h = int(hist[-1])
        return data[emit]


def slicer(x, T=0.0):
    return (x.astype(np.float64) > T).astype(np.uint8)


class DiffDecModel:
    def __init__(self, invert=False):
        self.invert, self.prev = invert, 0

    def process(self, x):
        x = np.asarray(x, np.uint8)
        prev = np.concatenate([[self.prev], x[:-1]]).astype(np.int64)
        v = prev ^ x.astype(np.int64)
        if len(x):
            self.prev = int(x[-1])
        return ((v + 1) % 2 if self.invert else v).astype(np.uint8)


class ClockSamplerModel:
    """sampler(data = x, clock = ZC(x)) [-> slicer [-> differential decoder]]"""

    def __init__(self, P, T=0.0, slice_t=None, invert=None):
        self.zc, self.sampler = ZcFast(P, T), SamplerFast()
        self.slice_t = slice_t
        self.dec = DiffDecModel(invert) if invert is not None else None

    def process(self, x):
        clk = np.where(self.zc.pulses(x), 1.0, -1.0).astype(np.float32)
        y = self.sampler.process(x, clk)
        if self.slice_t is None:
            return y
        b = slicer(y, self.slice_t)
        return self.dec.process(b) if self.dec is not None else b


def zc_advance(P, o, n):
    """the device fallback's walk (kernels_digital.h zc_advance): n literal samples from offset o, whole symbols at a time"""
    while n:
        if o >= 2.0:
            m = min(n, int(math.floor(o) - 1.0))
            o -= float(m)
            n -= m
        else:
            o = o - 1.0
            if o < 1.0:
                o = o + P
            n -= 1
    return o


class ZcJump:
    """the device fallback's scheme: the literal offset carried across calls and from tile start to tile start with zc_advance; each sample's
    pulse from the offset advanced to it.  Equal to ZcLiteral only if every jump is exact."""

    def __init__(self, P, T=0.0, tile=4096):
        self.P, self.T, self.tile = float(P), float(T), tile
        self.h, self.o = False, float(P)

    def process(self, x):
        P, T = self.P, self.T
        out = np.empty(len(x), np.float32)
        resets, h = [], self.h
        for i, v in enumerate(x.tolist()):
            if (not h and v > T) or (h and v < T):
                h = not h
                resets.append(i)
        # offsets at tile starts (the carry kernel), then each tile's samples from its start or its last reset
        o_tile, o, r = [], self.o, 0
        last = None
        for t0 in range(0, len(x), self.tile):
            o_tile.append(o)
            t1 = min(t0 + self.tile, len(x))
            rs = [c for c in resets if t0 <= c < t1]
            o = zc_advance(P, P / 2, t1 - rs[-1]) if rs else zc_advance(P, o, t1 - t0)
        rset = set(resets)
        for t, t0 in enumerate(range(0, len(x), self.tile)):
            oo = o_tile[t]
            for i in range(t0, min(t0 + self.tile, len(x))):
                if i in rset:
                    oo = P / 2
                oo = oo - 1.0
                if oo < 1.0:
                    out[i] = 1
                    oo = oo + P
                else:
                    out[i] = -1
        self.h, self.o = h, o
        return out
