"""CPU models of VaricodeDecoderBlock (radio/blocks/protocol/varicodedecoder.lua:61-87): the literal loop, the window-function automaton the
device runs (luaradio_amd/csrc/varicode_plan.h), an encoder, and the alphabet in the project's layout.

The literal loop appends every byte to a state; when the state's last two entries are 0 it looks the entries in front of them up (a byte
counts as a one only when it equals 1) and empties the state, else it empties the state once it holds more than 10 entries.  The automaton
keeps only the state's length and whether its last byte is 0 (21 states) and reads the looked-up bytes back from the stream.
"""
import numpy as np

# The PSK31 Varicode alphabet by character: CODE[c] read most significant bit first is the code of chr(c), without the 00 behind it
CODE = (
    0x2ab, 0x2db, 0x2ed, 0x377, 0x2eb, 0x35f, 0x2ef, 0x2fd, 0x2ff, 0x0ef, 0x01d, 0x36f, 0x2dd, 0x01f, 0x375, 0x3ab,
    0x2f7, 0x2f5, 0x3ad, 0x3af, 0x35b, 0x36b, 0x36d, 0x357, 0x37b, 0x37d, 0x3b7, 0x355, 0x35d, 0x3bb, 0x2fb, 0x37f,
    0x001, 0x1ff, 0x15f, 0x1f5, 0x1db, 0x2d5, 0x2bb, 0x17f, 0x0fb, 0x0f7, 0x16f, 0x1df, 0x075, 0x035, 0x057, 0x1af,
    0x0b7, 0x0bd, 0x0ed, 0x0ff, 0x177, 0x15b, 0x16b, 0x1ad, 0x1ab, 0x1b7, 0x0f5, 0x1bd, 0x1ed, 0x055, 0x1d7, 0x2af,
    0x2bd, 0x07d, 0x0eb, 0x0ad, 0x0b5, 0x077, 0x0db, 0x0fd, 0x155, 0x07f, 0x1fd, 0x17d, 0x0d7, 0x0bb, 0x0dd, 0x0ab,
    0x0d5, 0x1dd, 0x0af, 0x06f, 0x06d, 0x157, 0x1b5, 0x15d, 0x175, 0x17b, 0x2ad, 0x1f7, 0x1ef, 0x1fb, 0x2bf, 0x16d,
    0x2df, 0x00b, 0x05f, 0x02f, 0x02d, 0x003, 0x03d, 0x05b, 0x02b, 0x00d, 0x1eb, 0x0bf, 0x01b, 0x03b, 0x00f, 0x007,
    0x03f, 0x1bf, 0x015, 0x017, 0x005, 0x037, 0x07b, 0x06b, 0x0df, 0x05d, 0x1d5, 0x2b7, 0x1bb, 0x2b5, 0x2d7, 0x3b5)
BY_NUMBER = {code: c for c, code in enumerate(CODE)}
MAX_LEN = 10
TEN_BIT = tuple(c for c in range(128) if CODE[c] >= 0x200)       # the 40 characters the decoder never emits


def max_output(n):
    """the most characters a call of n bits emits (a character owns 3 bytes, its second zero lies in the call, the state carries 10 in)"""
    return min(n, (n + MAX_LEN) // 3)


def code_bits(c):
    """the code of character c (an int), most significant bit first"""
    return [int(b) for b in bin(CODE[c])[2:]]


def encode(text, idle=0, lead=2):
    """text (bytes / str / ints) -> uint8 bits: `lead` zeros, then per character its code, 00 and `idle` further zeros (an int, or one per character)"""
    if isinstance(text, str):
        text = text.encode("ascii")
    chars = list(text)
    idles = [idle] * len(chars) if isinstance(idle, int) else list(idle)
    bits = [0] * lead
    for c, extra in zip(chars, idles):
        bits += code_bits(c) + [0, 0] + [0] * extra
    return np.array(bits, np.uint8)


class VaricodeLiteral:
    """varicodedecoder.lua:61-87 line by line, the state a list of bytes carried across calls.  `positions` records, for every character since
    the last reset(), the index of the input byte that completed it (counted from that reset): the loop does not see where the calls are cut, so
    the characters of a call [a, b) of a longer stream are those with a <= position < b."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.state, self.positions, self.consumed = [], [], 0

    def process(self, x):
        out = []
        for at, b in enumerate(np.asarray(x, np.uint8).tolist(), self.consumed):
            self.state.append(b)
            if len(self.state) >= 2:
                if self.state[-2] == 0 and self.state[-1] == 0:
                    offset = 0 if self.state[0] == 1 else 1
                    number = 0
                    for v in self.state[offset:offset + max(len(self.state) - offset - 2, 0)]:      # Bit.tonumber(state, offset, length)
                        number = (number << 1) | (1 if v == 1 else 0)
                    if number in BY_NUMBER:
                        out.append(BY_NUMBER[number])
                        self.positions.append(at)
                    self.state = []
                elif len(self.state) > MAX_LEN:
                    self.state = []
        self.consumed += len(x)
        return np.array(out, np.uint8)


def state_index(length, last_zero):
    return 2 * (length - 1) + 1 + int(last_zero) if length else 0


def step(s, zero):
    """one byte from state s of the 21; returns (new state, L): L = the state's length at a delimiter, else 0"""
    length = (s + 1) // 2 + 1
    if zero and s and s % 2 == 0:
        return 0, length
    if length > MAX_LEN:
        return 0, 0
    return state_index(length, zero), 0


class VaricodeWindow:
    """the device's formulation: the 21-state automaton, and at a delimiter of length L the value of the L - 2 bytes in front of the two zeros,
    read back from the stream (the carried bytes, then the call's)"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.carried = []

    def process(self, x):
        stream = self.carried + np.asarray(x, np.uint8).tolist()
        s = state_index(len(self.carried), bool(self.carried) and self.carried[-1] == 0)
        out = []
        for u in range(len(self.carried), len(stream)):
            s, L = step(s, stream[u] == 0)
            if L:
                number = 0
                for v in stream[u - (L - 1):u - 1]:
                    number = (number << 1) | (1 if v == 1 else 0)
                if number in BY_NUMBER:
                    out.append(BY_NUMBER[number])
        length = (s + 1) // 2
        self.carried = stream[len(stream) - length:]
        return np.array(out, np.uint8)


def run_cuts(model, x, edges):
    """the model fed x[edges[k]:edges[k + 1]] call by call -> (all outputs, the count of every call)"""
    parts = [model.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), [len(p) for p in parts]
