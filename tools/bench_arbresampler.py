#!/usr/bin/env python3
"""Device throughput of ArbitraryResamplerBlock (luaradio_amd/csrc/kernels_arbresample.h) on one MI355X, on resident vectors: HIP-event timing on
the launch stream after a warm-up, as tools/bench_interleave.py.  2^log2-samples ComplexFloat32 input samples per call at ratios 48000/44100, 0.37
and 2.0, default options.  Two yardsticks are timed in the same process: RationalResamplerBlock(3, 2) on the same input, and per row a plain device
copy that reads and writes as many bytes in all as the row reads and writes ("of_copy" = copy ms / row ms).  One JSON object per row, appended to
--out (profiles/arbresampler_table.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = [("48000/44100", 48000 / 44100), ("0.37", 0.37), ("2.0", 2.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=26)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="append the rows to this file as well")
    args = ap.parse_args()
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types

    lr.init(0)
    lr.adopt_torch_stream()
    n = 1 << args.log2_samples

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def copy_ms(total_bytes):
        """a device copy that reads and writes total_bytes in all"""
        a = torch.empty(total_bytes // 2, dtype=torch.uint8, device="cuda").fill_(1)
        b = torch.empty_like(a)
        return timed(lambda: b.copy_(a))

    def ready(blk):
        blk.rate = 44100.0
        blk.differentiate([types.ComplexFloat32])
        blk.initialize()
        return blk

    x = torch.rand(2 * n, dtype=torch.float32, device="cuda") * 2 - 1

    def run(blk):
        """(ms per call of n resident input samples, outputs of the last call)"""
        cap = blk.max_output(n)
        y = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
        count = [0]

        def call():
            count[0] = blk.process_device(x.data_ptr(), n, y.data_ptr(), cap)
        return timed(call), count[0]

    rational_ms, rational_out = run(ready(lr.RationalResamplerBlock(3, 2)))
    rational_copy = copy_ms(8 * (n + rational_out))
    emit({"row": "rationalresampler", "L": 3, "D": 2, "samples": n, "outputs": rational_out, "ms": round(rational_ms, 4), "copy_ms": round(rational_copy, 4),
          "of_copy": round(rational_copy / rational_ms, 3), "Msps_in": round(n / rational_ms / 1e3, 1)})
    for name, ratio in RATIOS:
        blk = ready(lr.ArbitraryResamplerBlock(ratio))
        ms, outputs = run(blk)
        c = copy_ms(8 * (n + outputs))
        emit({"row": "arbresampler", "ratio": name, "phases": blk.phases, "taps_per_phase": blk.num_taps, "samples": n, "outputs": outputs, "ms": round(ms, 4),
              "copy_ms": round(c, 4), "of_copy": round(c / ms, 3), "Msps_in": round(n / ms / 1e3, 1), "rational_3_2_ms": round(rational_ms, 4),
              "TB/s": round(8 * (n + outputs) / (ms * 1e-3) / 1e12, 3)})
        del blk


if __name__ == "__main__":
    main()
