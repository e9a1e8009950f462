"""The default traceback depth of dvbs_fec_decoder per code rate, measured with the CPU models (tests/helpers/viterbi_model.py behind the depuncture
model of tests/helpers/fecglue_model.py): for each DVB-S rate, 2^18 + 1024 random message bits through the (7, [171, 133]) encoder and the puncturing
pattern, BPSK over AWGN at the Eb/N0 (searched in steps of 0.25 dB, then by bisection) where the bit error rate behind the windowed decoder at block 512, depth 256 is
about 1e-3, the same noise decoded at every depth 16, 32 .. 256.  The answer is the smallest depth whose error rate is within 10 % of the one at 256.
One JSON line per rate; DESIGN.md section 8 holds the table.

    python tools/dvbs_depth_table.py [--bits 263168] [--seed 7]
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import fecglue_model as fm  # noqa: E402
from tests.helpers import viterbi_model as vm  # noqa: E402

BLOCK, SCALE = 512, 8.0
START = {"1/2": 3.0, "2/3": 3.5, "3/4": 4.0, "5/6": 4.75, "7/8": 5.25}


def errors(q, message, depth):
    """bit errors of the windows the stream completes, and the bits compared"""
    got = vm.decode_windows(fm.K, fm.POLYS, q, BLOCK, depth)
    return int(np.count_nonzero(got != message[:len(got)])), len(got)


def measure(args):
    rate, nbits, seed = args
    pattern = fm.DVBS_PUNCTURE[rate]
    num, den = [int(v) for v in rate.split("/")]
    rng = np.random.default_rng(seed)
    message = rng.integers(0, 2, nbits).astype(np.uint8)
    sent = fm.puncture_model(pattern).process(vm.encode(fm.K, fm.POLYS, message))
    noise = np.random.default_rng(seed + 1).standard_normal(len(sent))

    def quantised(ebn0):
        sigma2 = 1.0 / (2.0 * (num / den) * 10.0 ** (ebn0 / 10.0))
        llr = (2.0 * ((1.0 - 2.0 * sent.astype(np.float64)) + np.sqrt(sigma2) * noise) / sigma2).astype(np.float32)
        return vm.quantise(fm.depuncture_model(pattern).process(llr), SCALE)

    def rate_at(ebn0):
        e, n = errors(quantised(ebn0), message, 256)
        return e / n

    # steps of 0.25 dB until 1e-3 is bracketed, then bisection
    ebn0, step, lo, hi = START[rate], 0.25, None, None             # lo: too many errors, hi: too few
    for _ in range(16):
        ber256 = rate_at(ebn0)
        if 0.8e-3 <= ber256 <= 1.25e-3:
            break
        if ber256 > 1e-3:
            lo = ebn0
        else:
            hi = ebn0
        ebn0 = (lo + hi) / 2 if lo is not None and hi is not None else ebn0 + (step if ber256 > 1e-3 else -step)
    q = quantised(ebn0)
    ber = {}
    for depth in range(16, 257, 16):
        e, n = errors(q, message, depth)
        ber[depth] = e / n
    chosen = min(d for d in ber if ber[d] <= 1.1 * ber[256])
    return {"rate": rate, "ebn0_db": ebn0, "message_bits": nbits, "ber_at_256": ber[256], "depth": chosen, "ber_at_depth": ber[chosen],
            "ber": {str(d): ber[d] for d in ber}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=(1 << 18) + 1024)       # 2^18 bits leave the decoder at every depth
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    jobs = [(rate, a.bits, a.seed) for rate in fm.DVBS_PUNCTURE]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        for row in pool.imap(measure, jobs):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
