#!/usr/bin/env python3
"""Device time of the PLL stage (luaradio_amd/csrc/kernels_pll.h) on one MI355X: the stereo pilot loop PLLBlock(100, 18950, 19050, 2) at 220 500 Hz on
resident ComplexFloat32 samples - a locked pilot in noise and pure noise - each on the default path (speculate / verify / repair) and with
speculate=0 (the serial recurrence in one lane, which is what the reference runs).  HIP-event timing on the launch stream, as tools/bench_digital.py;
the serial rows run once, without warm-up (they take seconds).  Prints one JSON object per row and appends it to --out; the ratio of the default to
the serial time on the locked signal is the figure of merit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--noise", type=float, default=0.3, help="sigma of the complex noise on the locked pilot, per component")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pll_table.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import blocks as B, types

    lr.init(0)
    lr.adopt_torch_stream()
    n = 1 << args.log2_samples
    rate = 220500.0
    rng = np.random.default_rng(1)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    pilot = (np.exp(1j * (2 * np.pi * (19000.0 / rate) * np.arange(n) + 1.0)) + args.noise * noise).astype(np.complex64)
    signals = {"locked pilot": torch.from_numpy(pilot).cuda(), "pure noise": torch.from_numpy(noise).cuda()}
    y = torch.empty(n, dtype=torch.complex64, device="cuda")
    rows = []
    for signal, x in signals.items():
        for path, knobs in (("default", ""), ("serial", ":speculate=0")):
            blk = B.PLLOutBlock(100, 18950, 19050, 2)
            blk.rate = rate
            blk.op_knobs = knobs
            blk.differentiate([types.ComplexFloat32])
            blk.initialize()
            ch = lr.Chain([blk])
            slow = path == "serial" or signal == "pure noise"        # out of lock the default path is the serial walk as well
            warmup, reps = (0, 1) if slow else (args.warmup, args.reps)
            for _ in range(warmup):
                ch.reset()
                ch.process_device(x.data_ptr(), n, y.data_ptr(), n)
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                ch.reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ch.process_device(x.data_ptr(), n, y.data_ptr(), n)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            row = {"row": "pll " + path, "signal": signal, "samples": n, "ms": round(min(ms), 3), "ms_all": [round(m, 3) for m in ms],
                   "launches": ch.last_launches, "msamples_per_s": round(n / (min(ms) * 1e-3) / 1e6, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    by = {(r["signal"], r["row"]): r["ms"] for r in rows}
    for signal in signals:
        row = {"row": "pll serial / default", "signal": signal, "samples": n, "ratio": round(by[(signal, "pll serial")] / by[(signal, "pll default")], 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
