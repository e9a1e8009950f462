#!/usr/bin/env python3
"""Device throughput of the digital tail (luaradio_amd/csrc/kernels_digital.h) on one MI355X: the fused clocksampler -> slicer -> differential
decoder chain and the clock recovery alone, on resident Float32 samples.  HIP-event timing on the launch stream after warm-up, as
tools/bench_blocks.py.  Prints one JSON object per row: ms per call, launches per call, and the fraction of 8 TB/s on the algorithmic bytes
(4 B/sample read; + 4 B/sample written for the clock recovery)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import _lib
    from luaradio_amd.blocks import digital_op

    lr.init(0)
    L = _lib.load()
    lr.adopt_torch_stream()
    n = 1 << args.log2_samples
    P = 1e6 / 80 / 1200
    rng = np.random.default_rng(1)
    sym = rng.choice([-1.0, 1.0], size=int(n / P) + 2)
    x = torch.from_numpy((np.repeat(sym, int(np.ceil(P)))[:n] + 0.3 * rng.standard_normal(n)).astype(np.float32)).cuda()
    rows = [("clocksampler+slicer+decoder", [digital_op("clocksampler", period=P, threshold=0.0), digital_op("slicer", threshold=0.0),
                                            "differentialdecoder:invert=1"], 1, 4.0),
            ("zerocrossingclockrecovery", [digital_op("zerocrossingclockrecovery", period=P, threshold=0.0)], 4, 8.0)]
    for name, ops, out_size, bytes_per in rows:
        stages = [_lib.check_ptr(L.lrhip_unary_create(o.encode(), 0.0, 0.0, 0, 0), o) for o in ops]
        ch = _lib.check_ptr(L.lrhip_chain_create((C.c_void_p * len(stages))(*stages), len(stages)), "chain")
        cap = L.lrhip_chain_max_output(ch, n)
        y = torch.empty(cap * out_size + 64, dtype=torch.uint8, device="cuda")
        for _ in range(args.warmup):
            _lib.check(L.lrhip_chain_execute_device(ch, x.data_ptr(), n, y.data_ptr(), cap), name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            m = _lib.check(L.lrhip_chain_execute_device(ch, x.data_ptr(), n, y.data_ptr(), cap), name)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        print(json.dumps({"row": name, "samples": n, "period": P, "ms": round(ms, 4), "outputs": int(m),
                          "launches": L.lrhip_chain_last_launches(ch), "roof_fraction": round(bytes_per * n / (ms * 1e-3) / 8e12, 3)}))
        L.lrhip_chain_destroy(ch)
        for s in stages:
            L.lrhip_stage_destroy(s)


if __name__ == "__main__":
    main()
