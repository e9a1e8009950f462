"""The contract of ReedSolomonEncoderBlock, ReedSolomonDecoderBlock, PackBitsBlock and UnpackBitsBlock as a literal model: one loop per rule.
None of the blocks exists in the reference; luaradio_amd/csrc/kernels_reedsolomon.h implements exactly this.

Field: GF(2^8) = GF(2)[x] / gfpoly in the polynomial basis, alpha = 2, tables by shift-and-reduce.  Code: g(x) = prod_{i < n - k} (x - alpha^((fcr + i)
prim)), byte j of a codeword is the coefficient of x^(n - 1 - j), the k message bytes first and unchanged, then the n - k bytes of (m(x) x^(n - k)) mod
g(x).  A shortened code (n < 255) has its 255 - n virtual zeros at the highest degrees.

Decoder: syndromes S_i = r(alpha^((fcr + i) prim)), Berlekamp-Massey, a Chien search over the n real positions, Forney with X = alpha^(prim p) for
degree p: e = X^(1 - fcr) Omega(1 / X) / Lambda'(1 / X).  Uncorrectable (status 255, the message bytes leave as received): the register length L of
Berlekamp-Massey (which bounds the locator's degree) exceeds t; the locator does not have exactly L roots among the n real positions; a magnitude is 0.

Frames: interleave = I, byte j of a frame belongs to codeword j mod I at index j div I; the encoder emits the I k message bytes as they came, then
the I (n - k) parity bytes interleaved the same way; the decoder emits the I k corrected message bytes and, with status, I status bytes."""
import numpy as np

UNCORRECTABLE = 255
# name -> (n, k, {gfpoly, fcr, prim}): where the kernels can go wrong (tests/test_gpu_reedsolomon.py says why each is there)
CCSDS = {"gfpoly": 0x187, "fcr": 112, "prim": 11}
PARAMETER_SETS = {"ccsds": (255, 223, CCSDS), "dvb": (204, 188, {}), "t32": (255, 191, {}), "t1-full": (255, 253, {}), "t1-short": (10, 8, {}),
                  "n63": (63, 47, {}), "n64": (64, 48, {}), "n65": (65, 49, {}), "general": (255, 239, {"gfpoly": 0x187, "fcr": 1})}
PRIMITIVE_POLYNOMIALS = (0x11d, 0x12b, 0x12d, 0x14d, 0x15f, 0x163, 0x165, 0x169, 0x171, 0x187, 0x18d, 0x1a9, 0x1c3, 0x1cf, 0x1e7, 0x1f5)


def gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def check_code(n, k, gfpoly=0x11d, fcr=0, prim=1, interleave=1):
    """the refusals of both blocks"""
    if not 3 <= n <= 255:
        raise ValueError("n must be 3 .. 255 (got %d)" % n)
    if not (1 <= k < n and (n - k) % 2 == 0 and 2 <= n - k <= 64):
        raise ValueError("k must be 1 .. n - 2 with n - k even and 2 .. 64 (got n = %d, k = %d)" % (n, k))
    if not Field.primitive(gfpoly):
        raise ValueError("gfpoly 0x%x is not a primitive polynomial of degree 8" % gfpoly)
    if not 0 <= fcr <= 254:
        raise ValueError("fcr must be 0 .. 254 (got %d)" % fcr)
    if not (1 <= prim <= 254 and gcd(prim, 255) == 1):
        raise ValueError("prim must be 1 .. 254 and coprime to 255 (got %d)" % prim)
    if not 1 <= interleave <= 8:
        raise ValueError("interleave must be 1 .. 8 (got %d)" % interleave)


class Field:
    @staticmethod
    def primitive(gfpoly):
        """degree 8, and alpha = 2 has order 255"""
        if not 0x100 <= gfpoly <= 0x1ff:
            return False
        x, seen = 1, set()
        for _ in range(255):
            if x == 0 or x in seen:
                return False
            seen.add(x)
            x <<= 1
            if x & 0x100:
                x ^= gfpoly
        return x == 1

    def __init__(self, gfpoly):
        assert Field.primitive(gfpoly)
        self.exp, self.log = [0] * 510, [None] * 256
        x = 1
        for i in range(255):
            self.exp[i] = self.exp[i + 255] = x
            self.log[x] = i
            x <<= 1
            if x & 0x100:
                x ^= gfpoly

    def mul(self, a, b):
        return 0 if a == 0 or b == 0 else self.exp[self.log[a] + self.log[b]]

    def div(self, a, b):
        assert b != 0
        return 0 if a == 0 else self.exp[self.log[a] + 255 - self.log[b]]

    def power(self, e):
        """alpha^e, any integer e"""
        return self.exp[e % 255]

    def evaluate(self, coefficients, x):
        """sum_i coefficients[i] x^i, by Horner from the top"""
        y = 0
        for c in reversed(coefficients):
            y = self.mul(y, x) ^ c
        return y


class Code:
    def __init__(self, n, k, gfpoly=0x11d, fcr=0, prim=1):
        check_code(n, k, gfpoly, fcr, prim)
        self.n, self.k, self.gfpoly, self.fcr, self.prim, self.t = n, k, gfpoly, fcr, prim, (n - k) // 2
        self.field = f = Field(gfpoly)
        self.roots = [f.power((fcr + i) * prim) for i in range(n - k)]
        g = [1]                                                   # g[j] = the coefficient of x^j
        for r in self.roots:
            g = [0] + g                                           # times x ...
            for j in range(len(g) - 1):
                g[j] ^= f.mul(g[j + 1], r)                        # ... plus r times the polynomial
        self.generator = g

    def parity(self, message):
        """(m(x) x^(n - k)) mod g(x) by long division: the n - k parity bytes, highest degree first"""
        f, g, p = self.field, self.generator, self.n - self.k
        assert len(message) == self.k
        rem = [int(v) for v in message] + [0] * p                 # highest degree first
        for i in range(self.k):
            lead = rem[i]
            if lead:
                for j in range(1, p + 1):
                    rem[i + j] ^= f.mul(lead, g[p - j])
        return rem[self.k:]

    def encode(self, message):
        return [int(v) for v in message] + self.parity(message)

    def syndromes(self, word):
        """S_i = r(root_i): byte j is the coefficient of x^(n - 1 - j)"""
        return [self.field.evaluate(list(reversed([int(v) for v in word])), r) for r in self.roots]

    def decode(self, word):
        """(the k message bytes, status): status = symbols corrected, 0 .. t, or UNCORRECTABLE with the received message bytes"""
        f, n, t = self.field, self.n, self.t
        word = [int(v) for v in word]
        assert len(word) == n
        S = self.syndromes(word)
        failed = (word[:self.k], UNCORRECTABLE)
        if not any(S):
            return word[:self.k], 0
        # Berlekamp-Massey: lam[i], prev[i] the coefficients of x^i
        lam, prev, L, b = [1] + [0] * (2 * t), [1] + [0] * (2 * t), 0, 1
        for r in range(2 * t):
            prev = [0] + prev[:-1]                                # x B
            d = 0
            for i in range(L + 1):
                if r - i >= 0:
                    d ^= f.mul(lam[i], S[r - i])
            if d:
                coefficient = f.div(d, b)
                old = list(lam)
                for i in range(2 * t + 1):
                    lam[i] ^= f.mul(coefficient, prev[i])
                if 2 * L <= r:
                    L, prev, b = r + 1 - L, old, d
        if L > t:
            return failed
        # Chien: the degrees p < n with Lambda(1 / X_p) = 0, X_p = alpha^(prim p)
        found = [p for p in range(n) if f.evaluate(lam[:L + 1], f.power(-self.prim * p)) == 0]
        if len(found) != L:
            return failed
        omega = [0] * L                                           # S(x) Lambda(x) mod x^L: deg Omega < L
        for j in range(L):
            for i in range(j + 1):
                omega[j] ^= f.mul(lam[i], S[j - i])
        derivative = [lam[i + 1] if i % 2 == 0 else 0 for i in range(L)]          # characteristic 2: the odd terms stay
        out = list(word)
        for p in found:
            inverse = f.power(-self.prim * p)
            num, den = f.evaluate(omega, inverse), f.evaluate(derivative, inverse)
            if num == 0 or den == 0:
                return failed
            e = f.mul(f.power(self.prim * p * (1 - self.fcr)), f.div(num, den))
            out[n - 1 - p] ^= e
        return out[:self.k], L


# ---- frames -----------------------------------------------------------------------------------------------------------------------------------------
def encode_frame(code, I, frame):
    """I k message bytes -> I n bytes"""
    frame = np.asarray(frame, np.uint8)
    assert len(frame) == I * code.k
    parity = np.zeros(I * (code.n - code.k), np.uint8)
    for c in range(I):
        parity[c::I] = code.parity(frame[c::I])
    return np.concatenate([frame, parity])


def decode_frame(code, I, frame, status):
    """I n received bytes -> I k message bytes (+ I status bytes)"""
    frame = np.asarray(frame, np.uint8)
    assert len(frame) == I * code.n
    out, flags = np.zeros(I * code.k, np.uint8), np.zeros(I, np.uint8)
    for c in range(I):
        out[c::I], flags[c] = code.decode(frame[c::I])
    return np.concatenate([out, flags]) if status else out


class FramedModel:
    """the streaming form of a stage that maps frames of fi bytes to frames of fo bytes: process() returns the frames its input completes, seek(n0)
    lands on frame n0 // fi with the bytes of that frame in front of n0 counted as zeros"""

    def __init__(self, fi, fo, function):
        self.fi, self.fo, self.function = fi, fo, function
        self.seek(0)

    def reset(self):
        self.seek(0)

    def seek(self, n0):
        self.Q = n0
        self.held = np.zeros(n0 % self.fi, np.uint8)
        return (n0 // self.fi) * self.fo

    def memory(self):
        return self.fi - 1

    def max_output(self, count):
        return -(-count // self.fi) * self.fo

    def process(self, x):
        self.held = np.concatenate([self.held, np.asarray(x, np.uint8)])
        self.Q += len(x)
        frames = len(self.held) // self.fi
        out = [self.function(self.held[f * self.fi:(f + 1) * self.fi]) for f in range(frames)]
        self.held = self.held[frames * self.fi:]
        return np.concatenate(out).astype(np.uint8) if out else np.zeros(0, np.uint8)


def encoder_model(n, k, gfpoly=0x11d, fcr=0, prim=1, interleave=1):
    check_code(n, k, gfpoly, fcr, prim, interleave)
    code = Code(n, k, gfpoly, fcr, prim)
    return FramedModel(interleave * k, interleave * n, lambda frame: encode_frame(code, interleave, frame))


def decoder_model(n, k, gfpoly=0x11d, fcr=0, prim=1, interleave=1, status=False):
    check_code(n, k, gfpoly, fcr, prim, interleave)
    code = Code(n, k, gfpoly, fcr, prim)
    return FramedModel(interleave * n, interleave * (k + (1 if status else 0)), lambda frame: decode_frame(code, interleave, frame, status))


# ---- bits <-> bytes ---------------------------------------------------------------------------------------------------------------------------------
def pack(bits, msb=True):
    """8 bits (bit 0 of each input byte) -> one byte, the first bit the most significant one with msb"""
    bits = np.asarray(bits, np.uint8) & 1
    assert len(bits) % 8 == 0
    out = np.zeros(len(bits) // 8, np.uint8)
    for i, b in enumerate(bits):
        out[i // 8] |= int(b) << ((7 - i % 8) if msb else i % 8)
    return out


def unpack(data, msb=True):
    data = np.asarray(data, np.uint8)
    out = np.zeros(8 * len(data), np.uint8)
    for i in range(len(out)):
        out[i] = (int(data[i // 8]) >> ((7 - i % 8) if msb else i % 8)) & 1
    return out


def pack_model(msb=True):
    return FramedModel(8, 1, lambda frame: pack(frame, msb))


def unpack_model(msb=True):
    return FramedModel(1, 8, lambda frame: unpack(frame, msb))
