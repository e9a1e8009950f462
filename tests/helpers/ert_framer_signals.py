"""The ERT receiver test signal of tests/helpers/ert_signals.py with *encoded* frames - valid SCM, SCM+ and IDM frames the framers accept - in
the same order (scm, scm+, idm, scm), with the same modulation, gaps, carrier offset and noise."""
import numpy as np

from tests.helpers import ert_framer_model as M
from tests.helpers.ert_signals import CHIP, ERT_ORDER, ERT_RATE


def encoded_frames(seed=11):
    """[(protocol, bits, the record fields sent)]"""
    rng = np.random.default_rng(seed)
    frames = []
    for proto in ERT_ORDER:
        bits, want = M.random_frame(M.PROTOCOLS[proto], rng)
        frames.append((proto, bits, want))
    return frames


def encoded_signal(sigma=0.05, seed=11):
    """four OOK frames (each bit b as the chips (b, 1 - b) of 72 samples) with 3 000 .. 9 000 samples of silence before each, 40 000 samples of
    tail, a carrier offset of 1 234.5 Hz and complex Gaussian noise of `sigma` per component.  Returns (x complex64, frames)."""
    frames = encoded_frames(seed)
    rng = np.random.default_rng(seed + 1)
    parts = []
    for _, bits, _ in frames:
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


def sent_records(frames):
    """{protocol: the records of its frames, in order}"""
    return {name: P.records([want for proto, _, want in frames if proto == name]) for name, P in M.PROTOCOLS.items()}
