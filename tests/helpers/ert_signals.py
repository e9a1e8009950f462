"""The ERT receiver test signal (shared by tests/test_ert_cpu.py and tests/test_gpu_ert.py) and the preamble sampler's random inputs."""
import numpy as np

from luaradio_amd import composites as comp

ERT_RATE, ERT_DECIMATION = 2359296.0, 6            # 393 216 S/s behind the downsampler: 24 samples per bit of 16 384 baud
ERT_ORDER = ("scm", "scm+", "idm", "scm")
CHIP = 72                                          # input samples per Manchester chip (rate / 32 768)


def ert_frames(seed=7):
    """[(protocol, bits)]: preamble + random payload, frame length of the protocol"""
    rng = np.random.default_rng(seed)
    frames = []
    for proto in ERT_ORDER:
        pre, n = comp.ERT_PROTOCOLS[proto]
        frames.append((proto, np.concatenate([np.array(pre, np.uint8), rng.integers(0, 2, n - len(pre)).astype(np.uint8)])))
    return frames


def ert_signal(sigma=0.05, seed=7):
    """four OOK frames (each bit b as the chips (b, 1 - b) of 72 samples) with 3 000 .. 9 000 samples of silence before each, 40 000 samples of
    tail, a carrier offset of 1 234.5 Hz and complex Gaussian noise of `sigma` per component.  Returns (x complex64, frames)."""
    frames = ert_frames(seed)
    rng = np.random.default_rng(seed + 1)
    parts = []
    for _, bits in frames:
        parts.append(np.zeros(int(rng.integers(3000, 9001))))
        chips = np.stack([bits, 1 - bits], axis=1).reshape(-1)
        parts.append(np.repeat(chips, CHIP).astype(np.float64))
    parts.append(np.zeros(40000))
    a = np.concatenate(parts)
    t = np.arange(len(a))
    x = a * np.exp(2j * np.pi * 1234.5 * t / ERT_RATE)
    if sigma:
        x = x + sigma * (rng.standard_normal(len(a)) + 1j * rng.standard_normal(len(a)))
    return x.astype(np.complex64), frames


def ert_expected(frames):
    """the Bit stream of each protocol's branch: its own frames, and on scm+ also bits 16 .. 143 of every IDM frame (the IDM preamble ends in
    the SCM+ preamble)"""
    want = {p: [] for p in comp.ERT_PROTOCOLS}
    for proto, bits in frames:
        want[proto].append(bits)
        if proto == "idm":
            want["scm+"].append(bits[16:16 + comp.SCM_PLUS_FRAME_LEN])
    return {p: (np.concatenate(v) if v else np.zeros(0, np.uint8)) for p, v in want.items()}


ALPHABET = np.array([1.0, -1.0, 0.5, -0.5, 0.25, 0.0, np.nan, np.inf, -np.inf, -0.0], np.float32)


def alphabet_signal(n, seed, weights=None):
    """samples from a small alphabet, so that ties in the energy and non-finite values are frequent"""
    rng = np.random.default_rng(seed)
    return ALPHABET[rng.choice(len(ALPHABET), size=n, p=weights)]


def plant_frame(x, at, T, preamble, N, rng, amp=1.0):
    """writes a frame of N symbols (preamble, then random bits) as +-amp levels of T samples at x[at:]; returns the end"""
    bits = np.concatenate([np.asarray(preamble, np.uint8), rng.integers(0, 2, max(N - len(preamble), 0)).astype(np.uint8)])[:max(N, len(preamble))]
    lv = np.repeat(np.where(bits > 0, amp, -amp), T).astype(np.float32)
    # a raised middle makes the energy peak inside each symbol
    lv *= np.tile(1.0 - 0.5 * np.abs(np.linspace(-1, 1, T)), len(bits)).astype(np.float32)
    end = min(at + len(lv), len(x))
    x[at:end] = lv[:end - at]
    return end


def ragged_cuts(n, frames, B, T, N, seed):
    """chunk edges: random, exactly at an i*, at a j*, one before and one after a j*, inside a frame, at s', two closer together than B, and a
    one-sample and a zero-length call (a repeated edge).  frames: [(i*, j*)] by absolute index."""
    rng = np.random.default_rng(seed)
    cuts = set(int(c) for c in rng.integers(1, max(n, 2), 6))
    if frames:
        picks = [frames[0], frames[len(frames) // 2], frames[-1]]
        for q, (i_star, j_star) in enumerate(picks):
            cuts |= [{i_star, j_star + (N - 1) * T}, {j_star, j_star + T + 1}, {j_star - 1, j_star + 1}][q % 3]
    mid = n // 2
    cuts |= {mid, mid + max(B // 3, 1), mid + max(B // 3, 1) + 1}
    edges = [0] + sorted(c for c in cuts if 0 < c < n) + [n]
    k = len(edges) // 2
    return edges[:k] + [edges[k]] + edges[k:]          # edges[k] twice: a zero-length call
