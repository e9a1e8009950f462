"""numpy restatement of PulseAmplitudeModulatorBlock / QuadratureAmplitudeModulatorBlock (radio/blocks/signal/pulseamplitudemodulator.lua,
quadratureamplitudemodulator.lua), independent of luaradio_amd, and the f64 model of a held symbol stream through a FIR (the loopback chains).

`literal_process` is the reference's loop bit by bit (process(), :69-87); `ModulatorModel.process` computes the same per call with array
operations so that the large GPU cases do not wait for a Python loop - tests/test_modulator_cpu.py holds the two together.
"""
import math

import numpy as np


def pam_table(levels):
    """_build_amplitudes (pulseamplitudemodulator.lua:47-55), rounded once to Float32 where initialize() stores it (:62)"""
    level = np.arange(levels)
    table = np.zeros(levels, np.float32)
    table[level ^ (level >> 1)] = ((2.0 * level - levels + 1) / math.sqrt((levels ** 2 - 1) / 3)).astype(np.float32)
    return table


def qam_table(points):
    """_build_constellation (quadratureamplitudemodulator.lua:47-67): ComplexFloat32(i, q) holds the integers exactly, scalar_div
    (complexfloat32.lua:141-143) computes real / scaling and imag / scaling in double and ComplexFloat32.new rounds each once to Float32"""
    bits = int(round(math.log2(points)))
    i_bits = (bits + 1) // 2
    q_bits = bits - i_bits
    point = np.arange(points)
    i_value, q_value = point >> q_bits, point & ((1 << q_bits) - 1)
    gray = ((i_value ^ (i_value >> 1)) << q_bits) | (q_value ^ (q_value >> 1))
    scaling = math.sqrt(2 * (points - 1) / 3)
    table = np.zeros(points, np.complex64)
    table.real[gray] = ((2.0 * i_value - (1 << i_bits) + 1) / scaling).astype(np.float32)
    table.imag[gray] = ((2.0 * q_value - (1 << q_bits) + 1) / scaling).astype(np.float32)
    return table


def symbol_value(bits, msb_first):
    """Bit.tonumber (radio/types/bit.lua:132-149): a bit counts only when its byte equals 1"""
    n, x = len(bits), 0
    for i, v in enumerate(bits):
        if v == 1:
            x |= (1 << (n - 1 - i)) if msb_first else (1 << i)
    return x


def literal_process(state, x, table, symbol_bits, period, msb_first):
    """process() of either block: `state` is the list of pending bits (changed in place); returns the output vector"""
    out = np.zeros(((len(state) + len(x)) // symbol_bits) * period, table.dtype)
    offset = 0
    for v in x:
        state.append(int(v))
        if len(state) == symbol_bits:
            out[offset:offset + period] = table[symbol_value(state, msb_first)]
            offset += period
            del state[:]
    return out


class ModulatorModel:
    def __init__(self, table, period, msb_first=True):
        self.table = np.asarray(table)
        self.bits = int(round(math.log2(len(self.table))))
        assert 1 << self.bits == len(self.table)
        self.period, self.msb_first = int(period), bool(msb_first)
        self.reset()

    def reset(self):
        self.state = np.zeros(0, np.uint8)

    def symbols(self, x):
        """the symbol values one call completes; the rest of the bits is carried"""
        stream = np.concatenate([self.state, np.asarray(x, np.uint8)])
        nsym = len(stream) // self.bits
        self.state = stream[nsym * self.bits:].copy()
        ones = (stream[:nsym * self.bits] == 1).reshape(nsym, self.bits).astype(np.int64)
        shifts = np.arange(self.bits - 1, -1, -1) if self.msb_first else np.arange(self.bits)
        return (ones << shifts).sum(axis=1)

    def process(self, x):
        return np.repeat(self.table[self.symbols(x)], self.period)


def random_bits(rng, n, junk=True):
    """Bit bytes 0 / 1, with bytes 2 and 255 mixed in (they count as 0)"""
    x = rng.integers(0, 2, n).astype(np.uint8)
    if junk and n:
        where = rng.random(n) < 0.1
        x[where] = rng.choice(np.array([2, 255], np.uint8), int(where.sum()))
    return x


def hold_fir_f64(held, taps, decimation=1):
    """the held symbol stream (any dtype) through the FIR `taps` in double, zero history, then every `decimation`-th sample from the first"""
    held = np.asarray(held)
    h = np.asarray(taps, np.float64)
    x = held.astype(np.complex128 if np.iscomplexobj(held) else np.float64)
    y = np.convolve(x, h)[:len(x)]
    return y[::decimation]
