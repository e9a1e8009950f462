"""numpy models of InterleaveBlock, DeinterleaveBlock and the WAV record conversion (radio/blocks/signal/interleave.lua, deinterleave.lua,
sources/wavfile.lua), and literal transcriptions of the reference's loops that the models and the device blocks are held to."""
import numpy as np

# radio/utilities/format_utils.lua:82-97, the three formats a WAV file uses (wavfile.lua:59-63)
WAV = {8: ("<u1", 127.5, 127.5), 16: ("<i2", 0.0, 32767.5), 32: ("<i4", 0.0, 2147483647.5)}


def interleave(xs):
    """out[N i + k] = in_k[i]"""
    xs = [np.asarray(x) for x in xs]
    return np.stack(xs, axis=1).reshape(-1) if len(xs[0]) else xs[0][:0].copy()


def deinterleave(x, N):
    """the whole stream at once: out_j[i] = in[N i + j], port j receives ceil((n - j) / N)"""
    x = np.asarray(x)
    return tuple(x[j::N].copy() for j in range(N))


class DeinterleaveLoop:
    """deinterleave.lua:49-63 transcribed literally: the carried index, the per-channel offset, the ceil() length, the element loop"""

    def __init__(self, N):
        self.N, self.index = N, 0

    def process(self, x):
        N, outs = self.N, []
        for i in range(1, N + 1):
            offset = ((i - 1) - self.index) % N
            length = max(0, int(np.ceil((len(x) - offset) / N)))
            out = np.empty(length, x.dtype)
            for j in range(length):
                out[j] = x[N * j + offset]
            outs.append(out)
        self.index = (self.index + len(x)) % N
        return tuple(outs)


def run_cuts(proc, x, cuts, N):
    """a stream in consecutive calls of the lengths `cuts`; the per-channel concatenation"""
    parts, a = [[] for _ in range(N)], 0
    for n in cuts:
        for k, y in enumerate(proc(x[a:a + n])):
            parts[k].append(y)
        a += n
    assert a == len(x)
    return tuple(np.concatenate(p) if p else x[:0] for p in parts)


def ragged_cuts(total, N, seed):
    """call lengths that sum to `total`: empty calls, calls shorter than N, single samples and long ones"""
    rng = np.random.default_rng(seed)
    cuts, left = [], total
    menu = [0, 1, N - 1, N, N + 1, 2 * N + 1, 7, 64, 257]
    while left:
        n = min(int(rng.choice(menu)), left)
        cuts.append(n)
        left -= n
    return cuts + [0]


def wav_unpack(raw, N, bits):
    """sources/wavfile.lua:235-239: out_k[i] = (raw[N i + k] - offset) / scale in double, rounded once to Float32; whole frames only"""
    dt, offset, scale = WAV[bits]
    v = np.frombuffer(raw, dt)
    v = v[:len(v) // N * N].astype(np.float64)
    y = ((v - offset) / scale).astype(np.float32)
    return tuple(y[k::N].copy() for k in range(N))


def reference_source_chunk(raw_values, N, offset=0.0, scale=1.0):
    """sources/wavfile.lua:232-242 transcribed literally for one chunk of len(raw_values) raw samples: the outputs are resized to
    num_samples / N and the frame loop runs `for i = 0, num_samples / N - 1` with the FRACTIONAL bound Lua gives it - floor(num_samples / N)
    frames are converted, the num_samples mod N samples behind them are dropped.  (Vector:resize of a fractional length keeps the integer part.)"""
    num_samples = len(raw_values)
    bound = num_samples / N - 1            # a Lua number, not an integer
    outs = [[] for _ in range(N)]
    i = 0
    while i <= bound:
        for j in range(1, N + 1):
            outs[j - 1].append((raw_values[i * N + (j - 1)] - offset) / scale)
        i += 1
    return outs
