#!/usr/bin/env python3
"""Device throughput of the many-ported stages (luaradio_amd/csrc/kernels_interleave.h) on one MI355X, on resident vectors: HIP-event
timing on the launch stream after a warm-up, as tools/bench_digital.py.  One JSON object per row, appended to --out
(profiles/interleave_table.jsonl):

  interleave / deinterleave   2^log2-frames frames, N = 2, 3, 8, Float32 and ComplexFloat32; yardstick: a plain device copy of the same
                              total bytes (read + written), timed right before the row; "of_copy" = copy ms / row ms
  interleave2-reg / -lds      the register-only kernel for two channels against the LDS transpose (LRHIP_INTERLEAVE2_REG, read when the
                              library first runs such a stage: the two forms are timed in two child processes)
  wavpack bits = 16           N = 1, 2; yardsticks: a store-only pass over the records it writes (fill_), a copy of its 6 bytes per sample, and
                              the unfused pair in the same run - the Interleave stage followed by the format_pack stage ("s16le"), 14 bytes per sample
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="append the rows to this file as well")
    ap.add_argument("--only-interleave2", action="store_true", help="the two-channel Interleave rows alone (the child of the A/B)")
    args = ap.parse_args()
    import torch
    import luaradio_amd as lr
    from luaradio_amd import _lib

    lr.init(0)
    L = _lib.load()
    lr.adopt_torch_stream()
    n = 1 << args.log2_frames

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

    def stage(op):
        return _lib.check_ptr(L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0), op)

    def copy_ms(total_bytes):
        """a device copy that reads and writes total_bytes in all"""
        a = torch.empty(total_bytes // 2, dtype=torch.uint8, device="cuda").fill_(1)
        b = torch.empty_like(a)
        return timed(lambda: b.copy_(a))

    def planar(N, size):
        return [torch.randn(n * size // 4, dtype=torch.float32, device="cuda") for _ in range(N)]

    def run_many_in(st, ports, out, cap):
        table = _lib.port_table([p.data_ptr() for p in ports])
        return lambda: _lib.check(L.lrhip_stage_execute_device(st, C.addressof(table), n, out.data_ptr(), cap), "execute")

    if args.only_interleave2:
        form = "reg" if os.environ.get("LRHIP_INTERLEAVE2_REG", "1") != "0" else "lds"
        for size in (4, 8):
            ports, out = planar(2, size), torch.empty(2 * n * size, dtype=torch.uint8, device="cuda")
            st = stage("interleave:channels=2:size=%d" % size)
            c = copy_ms(4 * n * size)
            ms = timed(run_many_in(st, ports, out, 2 * n))
            emit({"row": "interleave2-%s" % form, "size": size, "frames": n, "ms": round(ms, 4), "copy_ms": round(c, 4), "of_copy": round(c / ms, 3),
                  "TB/s": round(4 * n * size / (ms * 1e-3) / 1e12, 3)})
            L.lrhip_stage_destroy(st)
        return

    for size in (4, 8):
        for N in (2, 3, 8):
            total = 2 * N * n * size
            ports, inter = planar(N, size), torch.randn(N * n * size // 4, dtype=torch.float32, device="cuda")
            c = copy_ms(total)
            st = stage("interleave:channels=%d:size=%d" % (N, size))
            ms = timed(run_many_in(st, ports, inter, N * n))
            emit({"row": "interleave", "channels": N, "size": size, "frames": n, "ms": round(ms, 4), "copy_ms": round(c, 4), "of_copy": round(c / ms, 3),
                  "TB/s": round(total / (ms * 1e-3) / 1e12, 3)})
            L.lrhip_stage_destroy(st)
            c = copy_ms(total)
            st = stage("deinterleave:channels=%d:size=%d" % (N, size))
            table = _lib.port_table([p.data_ptr() for p in ports])
            ms = timed(lambda: _lib.check(L.lrhip_stage_execute_device(st, inter.data_ptr(), N * n, C.addressof(table), n), "execute"))
            emit({"row": "deinterleave", "channels": N, "size": size, "frames": n, "ms": round(ms, 4), "copy_ms": round(c, 4), "of_copy": round(c / ms, 3),
                  "TB/s": round(total / (ms * 1e-3) / 1e12, 3)})
            L.lrhip_stage_destroy(st)
            del ports, inter

    # the A/B of the two-channel form: the knob is read once per process
    for knob in ("0", "1"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only-interleave2", "--log2-frames", str(args.log2_frames), "--reps", str(args.reps),
               "--warmup", str(args.warmup)] + (["--out", args.out] if args.out else [])
        subprocess.run(cmd, env=dict(os.environ, LRHIP_INTERLEAVE2_REG=knob), check=True, timeout=300)

    for N in (1, 2):
        ports = [torch.rand(n, dtype=torch.float32, device="cuda") * 2 - 1 for _ in range(N)]
        rec = torch.empty(N * n, dtype=torch.int16, device="cuda")
        mid = torch.empty(N * n, dtype=torch.float32, device="cuda")
        fill = timed(lambda: rec.fill_(7))
        c = copy_ms(6 * N * n)
        st = stage("wavpack:channels=%d:bits=16" % N)
        fused = timed(run_many_in(st, ports, rec, n))
        pack = _lib.check_ptr(L.lrhip_format_pack_create(b"s16le", 0), "format_pack")
        il = stage("interleave:channels=%d:size=4" % max(N, 2)) if N > 1 else None
        table = _lib.port_table([p.data_ptr() for p in ports])

        def unfused():
            src = ports[0]
            if il:
                _lib.check(L.lrhip_stage_execute_device(il, C.addressof(table), n, mid.data_ptr(), N * n), "interleave")
                src = mid
            _lib.check(L.lrhip_stage_execute_device(pack, src.data_ptr(), N * n, rec.data_ptr(), N * n), "format_pack")
        pair = timed(unfused)
        emit({"row": "wavpack", "channels": N, "bits": 16, "frames": n, "ms": round(fused, 4), "store_only_ms": round(fill, 4), "copy6_ms": round(c, 4),
              "unfused_ms": round(pair, 4), "of_copy": round(c / fused, 3), "of_unfused": round(pair / fused, 3),
              "TB/s": round(6 * N * n / (fused * 1e-3) / 1e12, 3), "unfused": "interleave + format_pack(s16le)" if il else "format_pack(s16le) alone (one channel has nothing to interleave)"})
        L.lrhip_stage_destroy(st)
        L.lrhip_stage_destroy(pack)
        if il:
            L.lrhip_stage_destroy(il)


if __name__ == "__main__":
    main()
