"""CPU models of RDSFramerBlock (radio/blocks/protocol/rdsframer.lua:95-201) and the block / frame encoder its tests need.

  RDSFramerLiteral   the reference's loop as it is written: a 104-bit buffer that is filled, tested when full, emptied by an accepted frame and
                     shifted by one bit after a rejected one
  RDSFramerFast      the same function as two passes: V(s) = "the window at s holds four correctable blocks" for every position at once (one
                     syndrome per block start serves all five offsets, the syndrome being linear), then the hop - from the first unconsumed
                     bit q to the first s >= q with V(s), which emits and sets q = s + 104
  encode_block       check word = syndrome(data << 10) ^ offset, so that syndrome(block ^ offset) = 0
Frames are rows of four uint16 (types.RDSFrameType)."""
import numpy as np

FRAME_LEN, BLOCK_LEN = 104, 26
OFFSET_WORDS = {"A": 0x0fc, "B": 0x198, "C": 0x168, "Cp": 0x350, "D": 0x1b4}                 # rdsframer.lua:38-40
# rdsframer.lua:45-54: the rows of H^T by the bit of the block they belong to, 1 << 25 first
PARITY_ROWS = [0x077, 0x2e7, 0x3af, 0x30b, 0x359, 0x370, 0x1b8, 0x0dc, 0x06e, 0x037, 0x2c7, 0x3bf, 0x303,
               0x35d, 0x372, 0x1b9, 0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001]
PARITY_CHECK_MATRIX = {1 << (25 - k): row for k, row in enumerate(PARITY_ROWS)}
PARITY_CHECK_MATRIX[0] = 0x000
CORRECT_MATRIX = {row: mask for mask, row in PARITY_CHECK_MATRIX.items()}                    # rdsframer.lua:58-67: syndrome -> the bit in error
FRAME_DTYPE = np.dtype((np.uint16, (4,)))


def syndrome(v):
    s = 0
    for i in range(25, -1, -1):
        s ^= PARITY_CHECK_MATRIX[v & (1 << i)]
    return s


def correct_block(block_bits, offset_word):
    """rds_correct_block (:105-137): the corrected 26 bits, or None where the reference returns false"""
    s = syndrome(block_bits ^ offset_word)
    if s == 0:
        return block_bits
    if s in CORRECT_MATRIX:
        return block_bits ^ CORRECT_MATRIX[s]
    return None


def tonumber(bits):
    """Bit.tonumber, MSB first: a byte counts as 1 only when it equals 1 (bit.lua:141)"""
    x = 0
    for b in bits:
        x = (x << 1) | (1 if b == 1 else 0)
    return x


def check_window(window):
    """:163-183 on 104 bytes: the four data words, or None"""
    a = correct_block(tonumber(window[:BLOCK_LEN]), OFFSET_WORDS["A"])
    if a is None:                                    # (the reference computes all four before it looks; the answer is the same)
        return None
    blocks = [None] + [tonumber(window[BLOCK_LEN * k:BLOCK_LEN * (k + 1)]) for k in range(1, 4)]
    b = correct_block(blocks[1], OFFSET_WORDS["B"])
    c = correct_block(blocks[2], OFFSET_WORDS["C"])
    if c is None:
        c = correct_block(blocks[2], OFFSET_WORDS["Cp"])
    d = correct_block(blocks[3], OFFSET_WORDS["D"])
    if a is None or b is None or c is None or d is None:
        return None
    return [a >> 10, b >> 10, c >> 10, d >> 10]


def _frames(rows):
    return np.array(rows, np.uint16).reshape(len(rows), 4)


class RDSFramerLiteral:
    def __init__(self):
        self.reset()

    def reset(self):
        self.rds_frame, self.rds_frame_length = [0] * FRAME_LEN, 0

    def process(self, x):
        x = np.asarray(x, np.uint8).tolist()
        out, i = [], 0
        while i < len(x):
            if self.rds_frame_length < FRAME_LEN:
                n = min(FRAME_LEN - self.rds_frame_length, len(x) - i)
                self.rds_frame[self.rds_frame_length:self.rds_frame_length + n] = x[i:i + n]
                i, self.rds_frame_length = i + n, self.rds_frame_length + n
            elif self.rds_frame_length == FRAME_LEN:
                self.rds_frame[0:FRAME_LEN - 1] = self.rds_frame[1:FRAME_LEN]
                self.rds_frame[FRAME_LEN - 1] = x[i]
                i = i + 1
            if self.rds_frame_length == FRAME_LEN:
                words = check_window(self.rds_frame)
                if words is not None:
                    out.append(words)
                    self.rds_frame_length = 0
        return _frames(out)


# syndrome -> is it zero or one row (a single-bit error)
_CORRECTABLE = np.zeros(1024, bool)
_CORRECTABLE[list(CORRECT_MATRIX)] = True


def valid_windows(bits):
    """V(s) for s = 0 .. len(bits) - 104 from 0 / 1 values"""
    n = len(bits)
    if n < FRAME_LEN:
        return np.zeros(0, bool)
    nb = n - BLOCK_LEN + 1
    syn = np.zeros(nb, np.int64)
    for k, row in enumerate(PARITY_ROWS):
        syn ^= np.where(bits[k:k + nb] == 1, row, 0)
    ok = {name: _CORRECTABLE[syn ^ off] for name, off in OFFSET_WORDS.items()}
    nv = n - FRAME_LEN + 1
    return ok["A"][:nv] & ok["B"][26:26 + nv] & (ok["C"] | ok["Cp"])[52:52 + nv] & ok["D"][78:78 + nv]


class RDSFramerFast:
    def __init__(self):
        self.reset()

    def reset(self):
        self.carry = np.zeros(0, np.uint8)           # the bits since q

    def process(self, x):
        bits = np.concatenate([self.carry, (np.asarray(x, np.uint8) == 1).astype(np.uint8)])
        hits = np.flatnonzero(valid_windows(bits))
        out, q = [], 0
        while True:
            k = np.searchsorted(hits, q)
            if k == len(hits):
                break
            s = int(hits[k])
            out.append(check_window(bits[s:s + FRAME_LEN].tolist()))
            q = s + FRAME_LEN
        q = max(q, len(bits) - (FRAME_LEN - 1))      # every window that ends inside this call has been tested
        self.carry = bits[q:].copy()
        return _frames(out)


def encode_block(data, offset_word):
    v = (int(data) & 0xffff) << 10
    return v | (syndrome(v) ^ offset_word)


def encode_frame(words, c_prime=False):
    """four 16-bit data words -> 104 bits, MSB first; c_prime codes the third block with offset C'"""
    offsets = [OFFSET_WORDS["A"], OFFSET_WORDS["B"], OFFSET_WORDS["Cp" if c_prime else "C"], OFFSET_WORDS["D"]]
    bits = []
    for w, off in zip(words, offsets):
        v = encode_block(w, off)
        bits.extend((v >> (BLOCK_LEN - 1 - k)) & 1 for k in range(BLOCK_LEN))
    return np.array(bits, np.uint8)


def random_stream(n, seed, kinds=("clean", "one", "multi", "two", "cprime")):
    """n random bits with frames of the given kinds inserted at random gaps of 0 .. 300 bits, every kind at least once while there is room:
    clean, one flipped bit in one block, one flipped bit in each of several blocks (both are accepted and corrected), two flipped bits in one block
    (rejected), the third block coded with C'.  Returns (bits, [(start, kind, words)])."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    placed, at, k = [], int(rng.integers(0, 301)), 0
    while at + FRAME_LEN <= n:
        kind = kinds[k % len(kinds)] if k < len(kinds) else kinds[int(rng.integers(0, len(kinds)))]
        words = [int(w) for w in rng.integers(0, 1 << 16, 4)]
        f = encode_frame(words, c_prime=(kind == "cprime"))
        if kind == "one":
            f[int(rng.integers(0, FRAME_LEN))] ^= 1
        elif kind == "multi":
            for b in rng.choice(4, int(rng.integers(2, 5)), replace=False):
                f[BLOCK_LEN * int(b) + int(rng.integers(0, BLOCK_LEN))] ^= 1
        elif kind == "two":
            b = int(rng.integers(0, 4))
            while True:                              # (a pair whose syndrome is a third row would be "corrected" into another codeword,
                p0, p1 = (int(p) for p in rng.choice(BLOCK_LEN, 2, replace=False))      # and in the third block C' gets its try as well)
                s = PARITY_ROWS[p0] ^ PARITY_ROWS[p1]
                if not _CORRECTABLE[s] and not (b == 2 and _CORRECTABLE[s ^ OFFSET_WORDS["C"] ^ OFFSET_WORDS["Cp"]]):
                    break
            f[BLOCK_LEN * b + p0] ^= 1
            f[BLOCK_LEN * b + p1] ^= 1
        bits[at:at + FRAME_LEN] = f
        placed.append((at, kind, words))
        at += FRAME_LEN + int(rng.integers(0, 301))
        k += 1
    return bits, placed


def overlap_stream(d):
    """104 + d bits in which the windows at 0 and at d both have four all-zero syndromes: a solution of the 80 linear equations
    syndrome(block) = offset over GF(2), by Gaussian elimination.  Returns None when the system is inconsistent."""
    n = FRAME_LEN + d
    rows, rhs = [], []
    offsets = [OFFSET_WORDS["A"], OFFSET_WORDS["B"], OFFSET_WORDS["C"], OFFSET_WORDS["D"]]
    for start in (0, d):
        for b, off in enumerate(offsets):
            for j in range(10):                      # bit j of the block's syndrome
                eq = np.zeros(n, np.uint8)
                for k, row in enumerate(PARITY_ROWS):
                    eq[start + BLOCK_LEN * b + k] ^= (row >> j) & 1
                rows.append(eq)
                rhs.append((off >> j) & 1)
    m = np.concatenate([np.array(rows, np.uint8), np.array(rhs, np.uint8)[:, None]], axis=1)
    pivots, r = [], 0
    for c in range(n):
        p = next((i for i in range(r, len(m)) if m[i, c]), None)
        if p is None:
            continue
        m[[r, p]] = m[[p, r]]
        for i in range(len(m)):
            if i != r and m[i, c]:
                m[i] ^= m[r]
        pivots.append(c)
        r += 1
        if r == len(m):
            break
    if any(m[i, n] and not m[i, :n].any() for i in range(len(m))):
        return None
    x = np.zeros(n, np.uint8)                        # free variables 0
    for i, c in enumerate(pivots):
        x[c] = m[i, n]
    return x
