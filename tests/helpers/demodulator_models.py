"""The contract of PulseAmplitudeDemodulatorBlock / QuadratureAmplitudeDemodulatorBlock as numpy, independent of luaradio_amd: `literal_process` is one
loop over samples, table entries and bits with Float32 scalars; `DemodulatorModel.process` computes the same per call with array operations, so the GPU
cases do not wait for a Python loop.  tests/test_demodulator_cpu.py holds the two together.

All arithmetic is Float32, each operation rounded on its own: dr = x.re - c.re, di = x.im - c.im, d = fl(fl(dr dr) + fl(di di)); a real table (pam) has
d = fl(dr dr).
  hard, general form: best = +inf, value 0; for v = 0 .. 2^b - 1 in order, v is taken when d_v < best.
  hard, grid form (table[v] = (I[v >> qb], Q[v & (2^qb - 1)]); a real table is its own single axis): the same rule per axis on fl(dr dr) and on fl(di di),
    the two indices joined.
  soft: llr_k = fl(fl(m1_k - m0_k) w), m0_k / m1_k the minima of d over the entries with bit k clear / set, by the same comparison from +inf; in the grid
    form m = fl(min_i a_i + min_q b_q) with the axis of bit k restricted to its half.
Symbol s is decided on stream sample s P + offset and emitted by the call that delivers that sample; output positions are bits b-1 .. 0 with msb_first,
else 0 .. b-1.
"""
import math

import numpy as np

F = np.float32
INF = F(np.inf)


def scaled_table(table, scale):
    """the received constellation: per component Float32(double(entry) * scale), rounded once"""
    table = np.asarray(table)
    if np.iscomplexobj(table):
        t = np.asarray(table, np.complex64)
        out = np.zeros(len(t), np.complex64)
        out.real = (t.real.astype(np.float64) * float(scale)).astype(np.float32)
        out.imag = (t.imag.astype(np.float64) * float(scale)).astype(np.float32)
        return out
    return (np.asarray(table, np.float32).astype(np.float64) * float(scale)).astype(np.float32)


def symbol_bits(table):
    b = int(round(math.log2(len(table))))
    assert 1 << b == len(table)
    return b


def detect_grid(table):
    """the smallest qb in 0 .. b with table[v] == (I[v >> qb], Q[v & (2^qb - 1)]) bit for bit for every v, or None"""
    t = np.asarray(table, np.complex64)
    b = symbol_bits(t)
    re, im = t.real.copy().view(np.uint32), t.imag.copy().view(np.uint32)
    v = np.arange(len(t))
    for qb in range(b + 1):
        if np.array_equal(re, re[v >> qb << qb]) and np.array_equal(im, im[v & ((1 << qb) - 1)]):
            return qb
    return None


def symbols_before(n, period, offset):
    """symbols whose sample s P + offset lies below stream position n: ceil((n - offset) / P), 0 while n <= offset"""
    return 0 if n <= offset else -(-(n - offset) // period)


def bit_positions(b, msb_first):
    return list(range(b - 1, -1, -1)) if msb_first else list(range(b))


# ---------------------------------------------------------------------------------------------------- the literal loop
def _axes(table, grid):
    """(I axis, Q axis or None, qb) of a real table or of a complex table in the grid form"""
    if not np.iscomplexobj(table):
        return np.asarray(table, np.float32), None, 0
    t = np.asarray(table, np.complex64)
    return t.real[::1 << grid].copy(), t.imag[:1 << grid].copy(), grid


def _literal_argmin(ds):
    best, value = INF, 0
    for v, d in enumerate(ds):
        if d < best:
            best, value = d, v
    return value


def _literal_min(ds):
    best = INF
    for d in ds:
        if d < best:
            best = d
    return best


def literal_symbol(x, table, grid, soft, weight):
    """one sample -> the symbol value (hard) or the list of llr_k, k = 0 .. b - 1 (soft).  grid: None = the general form"""
    b = symbol_bits(table)
    w = F(weight)
    with np.errstate(all="ignore"):
        if grid is None:
            t = np.asarray(table, np.complex64)
            xr, xi = F(np.complex64(x).real), F(np.complex64(x).imag)
            ds = []
            for c in t:
                dr, di = F(xr - F(c.real)), F(xi - F(c.imag))
                ds.append(F(F(dr * dr) + F(di * di)))
            if not soft:
                return _literal_argmin(ds)
            out = []
            for k in range(b):
                m0 = _literal_min([d for v, d in enumerate(ds) if not (v >> k) & 1])
                m1 = _literal_min([d for v, d in enumerate(ds) if (v >> k) & 1])
                out.append(F(F(m1 - m0) * w))
            return out
        axis_i, axis_q, qb = _axes(table, grid)
        if axis_q is None:
            xr, xi = F(x), None
        else:
            xr, xi = F(np.complex64(x).real), F(np.complex64(x).imag)
        a = [F(F(xr - c) * F(xr - c)) for c in axis_i]
        q = [F(F(xi - c) * F(xi - c)) for c in axis_q] if axis_q is not None else None
        if not soft:
            return _literal_argmin(a) if q is None else (_literal_argmin(a) << qb) | _literal_argmin(q)
        out = []
        for k in range(b):
            if q is None:
                m0 = _literal_min([d for v, d in enumerate(a) if not (v >> k) & 1])
                m1 = _literal_min([d for v, d in enumerate(a) if (v >> k) & 1])
            elif k < qb:
                mi = _literal_min(a)
                m0 = F(mi + _literal_min([d for v, d in enumerate(q) if not (v >> k) & 1]))
                m1 = F(mi + _literal_min([d for v, d in enumerate(q) if (v >> k) & 1]))
            else:
                mq = _literal_min(q)
                m0 = F(_literal_min([d for v, d in enumerate(a) if not (v >> (k - qb)) & 1]) + mq)
                m1 = F(_literal_min([d for v, d in enumerate(a) if (v >> (k - qb)) & 1]) + mq)
            out.append(F(F(m1 - m0) * w))
        return out


def literal_process(pos, x, table, period, offset, msb_first, soft=False, weight=1.0, grid=None):
    """one call that starts at stream position `pos`: the output vector (Bit bytes or Float32 LLRs)"""
    b = symbol_bits(table)
    out = []
    for i, sample in enumerate(x):
        n = pos + i
        if n >= offset and (n - offset) % period == 0:
            r = literal_symbol(sample, table, grid, soft, weight)
            out.extend((r[k] if soft else (r >> k) & 1) for k in bit_positions(b, msb_first))
    return np.array(out, np.float32 if soft else np.uint8)


# ---------------------------------------------------------------------------------------------------- the same with array operations
def _sq(x, axis):
    d = x[:, None] - axis[None, :]
    return d * d


def _min(d, axis=1):
    """the minimum by `d < best` from +inf: NaN never wins"""
    return np.where(np.isnan(d), INF, d).min(axis=axis) if d.shape[axis] else np.full(d.shape[0], INF, np.float32)


def _argmin(d):
    return np.argmin(np.where(np.isnan(d), INF, d), axis=1)


def _bit_minima(d, k):
    v = np.arange(d.shape[1])
    return _min(d[:, (v >> k) & 1 == 0]), _min(d[:, (v >> k) & 1 == 1])


def decide(x, table, grid, soft, weight):
    """samples -> symbol values (hard), or an (n, b) Float32 array of llr_k, column k = bit k (soft)"""
    b = symbol_bits(table)
    w = F(weight)
    with np.errstate(all="ignore"):
        if grid is None:
            t = np.asarray(table, np.complex64)
            x = np.asarray(x, np.complex64)
            d = _sq(x.real, t.real) + _sq(x.imag, t.imag)
            assert d.dtype == np.float32
            if not soft:
                return _argmin(d)
            cols = [_bit_minima(d, k) for k in range(b)]
        else:
            axis_i, axis_q, qb = _axes(table, grid)
            if axis_q is None:
                a, q = _sq(np.asarray(x, np.float32), axis_i), None
            else:
                x = np.asarray(x, np.complex64)
                a, q = _sq(x.real, axis_i), _sq(x.imag, axis_q)
            if not soft:
                return _argmin(a) if q is None else (_argmin(a) << qb) | _argmin(q)
            if q is None:
                cols = [_bit_minima(a, k) for k in range(b)]
            else:
                mi, mq = _min(a), _min(q)
                cols = [tuple(mi + m for m in _bit_minima(q, k)) for k in range(qb)] + [tuple(m + mq for m in _bit_minima(a, k)) for k in range(b - qb)]
        out = np.stack([(m1 - m0) * w for m0, m1 in cols], axis=1) if len(x) else np.zeros((0, b), np.float32)
        assert out.dtype == np.float32
        return out


class DemodulatorModel:
    """grid: None = the general form, qb = the grid form; a real table (pam) is always its one axis"""

    def __init__(self, table, period, offset=0, msb_first=True, soft=False, weight=1.0, grid=None):
        self.table = np.asarray(table)
        self.b = symbol_bits(self.table)
        self.period, self.offset, self.msb_first, self.soft, self.weight = int(period), int(offset), bool(msb_first), bool(soft), F(weight)
        self.grid = 0 if not np.iscomplexobj(self.table) else grid
        self.pos = 0

    def reset(self):
        self.pos = 0

    def seek(self, n0):
        self.pos = int(n0)
        return symbols_before(self.pos, self.period, self.offset) * self.b

    def process(self, x):
        x = np.asarray(x)
        s0, s1 = (symbols_before(n, self.period, self.offset) for n in (self.pos, self.pos + len(x)))
        picked = x[np.arange(s0, s1) * self.period + self.offset - self.pos]
        self.pos += len(x)
        r = decide(picked, self.table, self.grid, self.soft, self.weight)
        ks = bit_positions(self.b, self.msb_first)
        if self.soft:
            return np.ascontiguousarray(r[:, ks]).reshape(-1)
        return ((r[:, None] >> np.array(ks)) & 1).astype(np.uint8).reshape(-1)


def same_floats(a, b):
    """bit equality of two Float32 vectors, a NaN matching any NaN (inf - inf has no payload worth a contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))
