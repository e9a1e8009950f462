"""The contract of ConvolutionalEncoderBlock and ViterbiDecoderBlock as a literal model: one loop per rule, and an array form of the decoder that the
tests hold to the loop bit for bit.  Neither block exists in the reference; luaradio_amd/csrc/kernels_viterbi.h implements exactly this.

Code: polynomials in the usual octal notation, bit K - 1 of g_j multiplies the current input bit.  r = (u_t << (K - 1)) | (r >> 1) from r = 0 at
absolute bit 0, out[n t + j] = parity(r & g_j), the state is r >> 1.

Decoder: q = clamp(rint(fl32(llr * scale)), -127, 127) once per input (Float32 product, ties to even, NaN -> 0), a hard bit b is q = 127 (1 - 2 b);
then int32 only.  Window w decodes the bits [w D, (w + 1) D) from the steps max(0, w D - L) .. (w + 1) D + L - 1 (Windows below)."""
import numpy as np

START_PENALTY = -(1 << 29)


def parity(v):
    return bin(v).count("1") & 1


def check_code(K, polys):
    """the refusals of both blocks, with their messages"""
    if not 3 <= K <= 9:
        raise ValueError("constraint length must be 3 .. 9 (got %d)" % K)
    if not 2 <= len(polys) <= 4:
        raise ValueError("the number of polynomials must be 2 .. 4 (got %d)" % len(polys))
    for g in polys:
        if g < 0 or g >> K:
            raise ValueError("polynomial %o (octal) has bits at or above the constraint length %d" % (g, K))
    if not any((g >> (K - 1)) & 1 for g in polys):
        raise ValueError("no polynomial has bit %d set" % (K - 1))
    if not any(g & 1 for g in polys):
        raise ValueError("no polynomial has bit 0 set")


class EncoderModel:
    def __init__(self, K, polys):
        check_code(K, polys)
        self.K, self.polys, self.n = K, list(polys), len(polys)
        self.reset()

    def reset(self):
        self.r = 0

    def seek(self, n0):
        self.r = 0
        return self.n * n0

    def process(self, bits):
        out = np.empty(len(bits) * self.n, np.uint8)
        for t, u in enumerate(np.asarray(bits, np.uint8)):
            self.r = ((int(u) & 1) << (self.K - 1)) | (self.r >> 1)
            for j, g in enumerate(self.polys):
                out[self.n * t + j] = parity(self.r & g)
        return out


def encode(K, polys, bits):
    return EncoderModel(K, polys).process(bits)


def quantise(llr, scale):
    """Float32 LLRs -> int32 in [-127, 127]: one Float32 product, rounded to nearest even, clamped; NaN is an erasure"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(llr, np.float32) * np.float32(scale))
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(-127), np.float32(127)))
    return v.astype(np.int32)


def quantise_bits(bits):
    return (127 * (1 - 2 * (np.asarray(bits, np.int32) & 1))).astype(np.int32)


# ---- counts (luaradio_amd/csrc/viterbi_plan.h) ------------------------------------------------------------------------------------------------------
def first_step(w, D, L):
    return max(0, w * D - L)


def last_step(w, D, L):
    return (w + 1) * D + L - 1


def windows_done(Q, n, D, L):
    E = Q // n
    return (E - L) // D if E >= L else 0


def bits_done(Q, n, D, L):
    return windows_done(Q, n, D, L) * D


def max_output(N, n, D, L):
    e = -(-N // n)                       # N inputs complete at most ceil(N / n) steps, e steps at most ceil(e / D) windows
    return -(-e // D) * D


def memory(n, D, L):
    return n * (D + 2 * L) - 1


# ---- one window, literally --------------------------------------------------------------------------------------------------------------------------
def decode_steps_loop(K, polys, q, known_start):
    """the steps q[0 : n T] of one window: returns the T bits of the traceback from the best final state"""
    n, S = len(polys), 1 << (K - 1)
    T = len(q) // n
    m = [0] * S
    if known_start:
        m = [0] + [START_PENALTY] * (S - 1)
    dec = []
    for t in range(T):
        qs = [int(v) for v in q[n * t:n * t + n]]
        new, d = [0] * S, [0] * S
        for s in range(S):
            u = s >> (K - 2)
            cand = []
            for b in (0, 1):
                p = ((s << 1) | b) & (S - 1)
                reg = (u << (K - 1)) | p
                bm = sum(-qs[j] if parity(reg & g) else qs[j] for j, g in enumerate(polys))
                cand.append(m[p] + bm)
            d[s] = int(cand[1] > cand[0])
            new[s] = max(cand)
        m = new
        dec.append(d)
    s = max(range(S), key=lambda i: (m[i], -i))
    bits = np.zeros(T, np.uint8)
    for t in range(T - 1, -1, -1):
        bits[t] = s >> (K - 2)
        s = ((s << 1) | dec[t][s]) & (S - 1)
    return bits


class Trellis:
    """the same window with one numpy operation per step"""

    def __init__(self, K, polys):
        n, S = len(polys), 1 << (K - 1)
        s = np.arange(S)
        self.K, self.n, self.S = K, n, S
        self.pred = np.stack([((s << 1) | b) & (S - 1) for b in (0, 1)])                                     # [b][s]
        reg = ((s >> (K - 2)) << (K - 1))[None, :] | self.pred
        par = np.array([[[parity(int(r) & g) for r in reg[b]] for b in (0, 1)] for g in polys])           # [j][b][s]
        self.sign = (1 - 2 * par).astype(np.int32)

    def decode_steps(self, q, known_start):
        n, S, K = self.n, self.S, self.K
        T = len(q) // n
        q = np.asarray(q[:n * T], np.int32).reshape(T, n)
        m = np.zeros(S, np.int32)
        if known_start:
            m[1:] = START_PENALTY
        dec = np.empty((T, S), np.uint8)
        for t in range(T):
            bm = np.tensordot(q[t], self.sign, axes=(0, 0))                                                  # [b][s]
            cand = m[self.pred] + bm
            dec[t] = cand[1] > cand[0]
            m = np.maximum(cand[0], cand[1]).astype(np.int32)
        s = int(np.argmax(m))                                                                                # the first, that is the lowest, maximum
        bits = np.empty(T, np.uint8)
        for t in range(T - 1, -1, -1):
            bits[t] = s >> (K - 2)
            s = ((s << 1) | int(dec[t, s])) & (S - 1)
        return bits


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------------
def decode_windows(K, polys, q, D, L, literal=False, first_window=0, q_start=0):
    """every complete window of the quantised stream q, whose element 0 is absolute input q_start (inputs in front of it do not exist: a caller that
    wants erasures there passes zeros); returns the bits of windows first_window .. windows_done - 1"""
    n = len(polys)
    trellis = None if literal else Trellis(K, polys)
    out = []
    for w in range(first_window, windows_done(q_start + len(q), n, D, L)):
        t0, t1 = first_step(w, D, L), last_step(w, D, L)
        seg = q[n * t0 - q_start:n * (t1 + 1) - q_start]
        assert n * t0 >= q_start and len(seg) == n * (t1 - t0 + 1)
        bits = decode_steps_loop(K, polys, seg, t0 == 0) if literal else trellis.decode_steps(seg, t0 == 0)
        out.append(bits[w * D - t0:w * D - t0 + D])
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def decode_full(K, polys, q):
    """one window over the whole stream: the full-sequence decoder with the same quantisation and tie rules"""
    return Trellis(K, polys).decode_steps(q, True)


class DecoderModel:
    """the streaming block: process() returns the windows its inputs complete, seek() leaves the carried inputs as erasures"""

    def __init__(self, K, polys, soft=True, scale=8.0, block=512, depth=None, literal=False):
        check_code(K, polys)
        self.K, self.polys, self.n, self.soft, self.scale = K, list(polys), len(polys), soft, scale
        self.D, self.L, self.literal = block, 8 * (K - 1) if depth is None else depth, literal
        self.seek(0)

    def reset(self):
        self.seek(0)

    def seek(self, n0):
        self.Q, self.done = n0, windows_done(n0, self.n, self.D, self.L)
        self.base = self.n * first_step(self.done, self.D, self.L)
        self.q = np.zeros(n0 - self.base, np.int32)
        return self.done * self.D

    def process(self, x):
        new = quantise(x, self.scale) if self.soft else quantise_bits(x)
        self.q = np.concatenate([self.q, new])
        self.Q += len(new)
        out = decode_windows(self.K, self.polys, self.q, self.D, self.L, self.literal, self.done, self.base)
        self.done = windows_done(self.Q, self.n, self.D, self.L)
        base = self.n * first_step(self.done, self.D, self.L)
        self.q = self.q[base - self.base:]
        self.base = base
        return out


def awgn_llrs(rng, code_bits, ebn0_db, rate):
    """BPSK over AWGN, unit symbol energy: the LLRs 2 y / sigma^2 as Float32, positive = 0"""
    sigma2 = 1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0))
    y = (1.0 - 2.0 * np.asarray(code_bits, np.float64)) + np.sqrt(sigma2) * rng.standard_normal(len(code_bits))
    return (2.0 * y / sigma2).astype(np.float32)
