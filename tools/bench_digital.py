#!/usr/bin/env python3
"""Device throughput of the digital tail (luaradio_amd/csrc/kernels_digital.h) on one MI355X: the fused clocksampler -> slicer -> differential
decoder chain and the clock recovery alone, on resident Float32 samples; the binary phase corrector (kernels_phasecorr.h) alone on resident
ComplexFloat32 samples next to a copy of the same buffer (16 B/sample); and the three digital receivers up to their bit streams.  HIP-event timing on the launch stream after warm-up, as
tools/bench_blocks.py.  Prints one JSON object per row: ms per call, launches per call, and the fraction of 8 TB/s on the algorithmic bytes
(4 B/sample read; + 4 B/sample written for the clock recovery).  --modulators, --ert-framers and --packet-framers print the rows of the
PAM / QAM modulators, of the SCM / SCM+ / IDM framers, of the AX.25 / POCSAG framers and of the Varicode decoder instead (modulator_rows,
ert_framer_rows, packet_framer_rows, varicode_rows); --demodulators prints the rows of the PAM / QAM demodulators (demodulator_rows); --fec those of
the convolutional encoder and the Viterbi decoder (fec_rows); --reed-solomon those of the Reed-Solomon encoder and decoder (reed_solomon_rows);
--fecglue those of the puncturing, interleaving and scrambling stages and of the two DVB-S FEC chains (fecglue_rows)."""
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
    ap.add_argument("--modulators", action="store_true", help="only the PAM / QAM modulator rows (profiles/modulator_table.jsonl)")
    ap.add_argument("--demodulators", action="store_true", help="only the PAM / QAM demodulator rows (profiles/demodulator_table.jsonl)")
    ap.add_argument("--ert-framers", action="store_true", help="only the SCM / SCM+ / IDM framer rows (profiles/ert_framer_table.jsonl)")
    ap.add_argument("--packet-framers", action="store_true", help="only the AX.25 / POCSAG framer rows (profiles/packet_framer_table.jsonl)")
    ap.add_argument("--varicode", action="store_true", help="only the Varicode decoder rows (profiles/varicode_table.jsonl)")
    ap.add_argument("--fec", action="store_true", help="only the convolutional encoder / Viterbi decoder rows (profiles/fec_table.jsonl)")
    ap.add_argument("--reed-solomon", action="store_true", help="only the Reed-Solomon encoder / decoder rows (appended to profiles/fec_table.jsonl)")
    ap.add_argument("--fecglue", action="store_true", help="only the puncture / depuncture / interleaver / scrambler / DVB-S chain rows (appended to "
                                                           "profiles/fec_table.jsonl)")
    ap.add_argument("--out", help="with --modulators / --demodulators / --ert-framers / --packet-framers / --varicode / --fec / --reed-solomon / --fecglue: append the rows to this "
                                  "file as well")
    args = ap.parse_args()
    if args.modulators:
        return modulator_rows(args)
    if args.demodulators:
        return demodulator_rows(args)
    if args.ert_framers:
        return ert_framer_rows(args)
    if args.packet_framers:
        return packet_framer_rows(args)
    if args.varicode:
        return varicode_rows(args)
    if args.fec:
        return fec_rows(args)
    if args.reed_solomon:
        return reed_solomon_rows(args)
    if args.fecglue:
        return fecglue_rows(args)
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

    # ---- the binary phase corrector: 8 B/sample read + 8 B/sample written, plus one strided 8-B read per measurement
    xc = torch.from_numpy((rng.standard_normal(2 * n).astype(np.float32))).cuda().view(torch.complex64)
    yc = torch.empty_like(xc)

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

    ms = timed(lambda: yc.copy_(xc))
    print(json.dumps({"row": "copy 16 B/sample (same buffers)", "samples": n, "ms": round(ms, 4), "roof_fraction": round(16.0 * n / (ms * 1e-3) / 8e12, 3)}))
    for N, I in [(3000, 32), (50, 32)]:
        op = digital_op("binaryphasecorrector", num_samples=N, sample_interval=I)
        st = _lib.check_ptr(L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 1), op)
        ms = timed(lambda: _lib.check(L.lrhip_stage_execute_device(st, xc.data_ptr(), n, yc.data_ptr(), n), op))
        print(json.dumps({"row": "binaryphasecorrector N=%d I=%d" % (N, I), "samples": n, "ms": round(ms, 4),
                          "roof_fraction": round((16.0 + 8.0 / I) * n / (ms * 1e-3) / 8e12, 3)}))
        L.lrhip_stage_destroy(st)

    # ---- the receivers, input resident on the device (the POCSAG graph takes host vectors: its time includes the copies in and out)
    m = min(n, 1 << 24)
    out = torch.empty(m + 64, dtype=torch.uint8, device="cuda")
    for name, rx, rate in [("ax25_receiver", lr.ax25_receiver(), 1e6), ("bpsk31_receiver", lr.bpsk31_receiver(1000.0), 1000.0)]:
        cap = rx.max_output(m)
        ms = timed(lambda: rx.process_device(xc.data_ptr(), m, out.data_ptr(), cap))
        print(json.dumps({"row": name, "samples": m, "rate": rate, "ms": round(ms, 4), "launches": rx.chain.last_launches,
                          "MS/s": round(m / ms / 1e3, 1)}))
    g = lr.pocsag_receiver()
    xh = xc[:m].cpu().numpy()
    ms = timed(lambda: g.process(**{"in": xh}))
    print(json.dumps({"row": "pocsag_receiver (host vectors)", "samples": m, "rate": 1e6, "ms": round(ms, 4), "MS/s": round(m / ms / 1e3, 1)}))


def modulator_rows(args):
    """The stand-alone modulators at 2^log2-samples OUTPUT samples (the kernels are bound by their stores), each next to a store-only pass over
    exactly the bytes it writes (torch's fill_ on the same buffer: a yardstick for the store stream, not one of the library's kernels), the two
    alternating three times; and QAM(4), 8 samples per symbol -> RootRaisedCosineFilterBlock(129 taps) at 2^(log2-samples - 2) output samples as a
    Chain.  --out appends the rows to a file (profiles/modulator_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(1)

    def emit(row):
        line = json.dumps(row)
        print(line)
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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    def made(blk, in_type, rate):
        blk.rate = rate
        blk.differentiate([in_type])
        blk.initialize()
        return blk

    n_out = 1 << args.log2_samples
    for cls, count, period, out_size in [(lr.PulseAmplitudeModulatorBlock, 4, 8, 4), (lr.QuadratureAmplitudeModulatorBlock, 4, 8, 8),
                                         (lr.PulseAmplitudeModulatorBlock, 4, 1, 4), (lr.QuadratureAmplitudeModulatorBlock, 4, 1, 8)]:
        bits = 2 * (n_out // period)
        x = torch.from_numpy(rng.integers(0, 2, bits).astype(np.uint8)).cuda()
        y = torch.empty(n_out * out_size // 4, dtype=torch.float32, device="cuda")
        blk = made(cls(1.0, float(period), count), types.Bit, 1.0)
        ms, ms_store = [], []
        for _ in range(3):
            ms.append(timed(lambda: blk.process_device(x.data_ptr(), bits, y.data_ptr(), n_out)))
            ms_store.append(timed(lambda: y.fill_(1.0)))
        emit({"row": "%s(%d) P=%d" % (cls.name, count, period), "outputs": n_out, "ms": ms, "store_only_ms": ms_store,
              "share_of_store_only": round(min(ms_store) / min(ms), 3), "roof_fraction": round((n_out * out_size + bits) / (min(ms) * 1e-3) / 8e12, 3)})
    m_out, period = n_out >> 2, 8
    bits = 2 * (m_out // period)
    x = torch.from_numpy(rng.integers(0, 2, bits).astype(np.uint8)).cuda()
    y = torch.empty(2 * m_out + 64, dtype=torch.float32, device="cuda")
    chain = lr.Chain([made(lr.QuadratureAmplitudeModulatorBlock(1.0, float(period), 4), types.Bit, 1.0),
                      made(lr.RootRaisedCosineFilterBlock(129, 0.35, 1.0), types.ComplexFloat32, float(period))])
    cap = chain.max_output(bits)
    ms = [timed(lambda: chain.process_device(x.data_ptr(), bits, y.data_ptr(), cap)) for _ in range(3)]
    emit({"row": "QAM(4) P=8 -> RRC(129)", "outputs": m_out, "ms": ms, "launches": chain.last_launches, "GS/s": round(m_out / min(ms) / 1e6, 2)})


def demodulator_rows(args):
    """The stand-alone demodulators on 2^24 resident symbols, one sample per symbol (the kernels read 4 or 8 bytes and write b bytes, or 4 b with soft,
    per symbol) - each next to a read-only pass over the same input bytes (torch's sum: a yardstick for the load stream, not one of the library's
    kernels), the two alternating three times.  QAM-256 runs in its grid form and forced through the general search (grid=-1).  A record, not an
    acceptance criterion.  --out appends the rows to a file (profiles/demodulator_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import _lib, types

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(1)
    n = 1 << 24

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    psk8 = [complex(np.cos(2 * np.pi * k / 8), np.sin(2 * np.pi * k / 8)) for k in range(8)]
    rows = [("QAM-16 hard", lr.QuadratureAmplitudeDemodulatorBlock, 16, {}, False),
            ("QAM-256 hard, grid", lr.QuadratureAmplitudeDemodulatorBlock, 256, {}, False),
            ("QAM-256 hard, general", lr.QuadratureAmplitudeDemodulatorBlock, 256, {}, True),
            ("QAM-256 soft, grid", lr.QuadratureAmplitudeDemodulatorBlock, 256, {"soft": True}, False),
            ("QAM-256 soft, general", lr.QuadratureAmplitudeDemodulatorBlock, 256, {"soft": True}, True),
            ("8-PSK hard (custom table)", lr.QuadratureAmplitudeDemodulatorBlock, 8, {"constellation": psk8}, False),
            ("PAM-4 hard", lr.PulseAmplitudeDemodulatorBlock, 4, {}, False)]
    for name, cls, count, options, general in rows:
        blk = cls(1.0, 1.0, count, options)
        blk.rate = 1.0
        cplx = cls is lr.QuadratureAmplitudeDemodulatorBlock
        blk.differentiate([types.ComplexFloat32 if cplx else types.Float32])
        if general:
            blk._set_stage(_lib.load().lrhip_unary_create(blk.op(grid=-1).encode(), 0.0, 0.0, 0, 0), "Creating a qamdemod stage with grid=-1")
        else:
            blk.initialize()
        table = blk.received_table()
        words = 2 if cplx else 1
        noise = 0.1 * rng.standard_normal(n * words).astype(np.float32)
        x = torch.from_numpy(table[rng.integers(0, count, n)].view(np.float32) + noise).cuda()
        bits = count.bit_length() - 1
        out_size = 4 if blk.soft else 1
        cap = blk.max_output(n)
        y = torch.empty(cap * out_size + 64, dtype=torch.uint8, device="cuda")
        ms, ms_read = [], []
        for _ in range(3):
            blk.reset()
            ms.append(timed(lambda: blk.process_device(x.data_ptr(), n, y.data_ptr(), cap)))
            ms_read.append(timed(lambda: x.sum()))
        row = {"row": name, "symbols": n, "op": blk.op(grid=-1 if general else None).split(":table=")[0], "ms": ms, "read_only_ms": ms_read,
               "share_of_read_only": round(min(ms_read) / min(ms), 3), "Gsymbol/s": round(n / min(ms) / 1e6, 2),
               "roof_fraction": round(n * (4 * words + bits * out_size) / (min(ms) * 1e-3) / 8e12, 3)}
        line = json.dumps(row)
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


def fec_rows(args):
    """ConvolutionalEncoderBlock and ViterbiDecoderBlock on resident vectors, 2^24 decoded (or message) bits per call: the encoder, the K = 7
    (171, 133) soft decoder at its default block of 512 and at 256 and 1024 (the LDS a window takes, and with it the resident waves, goes with the
    block), the same on hard bits, and the K = 9 (561, 753) soft decoder - each next to a read-only pass over the same input bytes (torch's sum, as in
    demodulator_rows), the two alternating three times.  Successive calls continue one stream, so every timed call decodes exactly 2^24 / D windows.
    A record, not an acceptance criterion.  --out appends the rows to a file (profiles/fec_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(1)
    nbits = 1 << 24

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    k7, k9 = [0o171, 0o133], [0o561, 0o753]
    rows = [("ConvolutionalEncoder K=7", lr.ConvolutionalEncoderBlock, (7, k7), types.Bit),
            ("Viterbi K=7 soft, block 512", lr.ViterbiDecoderBlock, (7, k7, {}), types.Float32),
            ("Viterbi K=7 soft, block 256", lr.ViterbiDecoderBlock, (7, k7, {"block": 256}), types.Float32),
            ("Viterbi K=7 soft, block 1024", lr.ViterbiDecoderBlock, (7, k7, {"block": 1024}), types.Float32),
            ("Viterbi K=7 hard, block 512", lr.ViterbiDecoderBlock, (7, k7, {"soft": False}), types.Bit),
            ("Viterbi K=9 soft, block 512", lr.ViterbiDecoderBlock, (9, k9, {}), types.Float32),
            ("Viterbi K=9 soft, block 256", lr.ViterbiDecoderBlock, (9, k9, {"block": 256}), types.Float32)]
    for name, cls, arguments, in_type in rows:
        blk = cls(*arguments)
        blk.rate = 1.0
        blk.differentiate([in_type])
        blk.initialize()
        decoder = cls is lr.ViterbiDecoderBlock
        n_in = nbits * len(blk.polynomials) if decoder else nbits
        if in_type is types.Float32:
            x = torch.from_numpy((2.0 * rng.standard_normal(n_in)).astype(np.float32)).cuda()
        else:
            x = torch.from_numpy(rng.integers(0, 2, n_in).astype(np.uint8)).cuda()
        cap = blk.max_output(n_in)
        y = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
        ms, ms_read = [], []
        for _ in range(3):
            blk.reset()
            ms.append(timed(lambda: blk.process_device(x.data_ptr(), n_in, y.data_ptr(), cap)))
            ms_read.append(timed(lambda: x.sum()))
        row = {"row": name, "bits": nbits, "op": blk.op(), "ms": ms, "read_only_ms": ms_read, "share_of_read_only": round(min(ms_read) / min(ms), 3),
               "Gbit/s": round(nbits / min(ms) / 1e6, 2)}
        if decoder:
            K, steps = blk.constraint_length, blk.block + 2 * blk.depth
            row["lds_bytes_per_wave"] = (steps + 63) // 64 * 64 * 8 * max(1, (1 << (K - 1)) // 64)
        line = json.dumps(row)
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


def reed_solomon_rows(args):
    """ReedSolomonEncoderBlock and ReedSolomonDecoderBlock (status bytes on) on resident vectors, about 2^24 message bytes per call in whole frames:
    CCSDS (255, 223) at I = 1 and I = 5 and DVB-S (204, 188); per code the encoder, the decoder on a clean stream, with t errors in one codeword of
    100, and with t errors in every codeword.  The decoder's input is the device encoder's output, the errors are put in on the host.  Each row
    stands next to a device-to-device copy that moves the row's input plus output bytes (a buffer of half that size copied once), the two
    alternating three times.  A record, not an acceptance criterion: the all-errors rows have no outside reference.  --out appends the rows to a
    file (profiles/fec_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(2)

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    def make(cls, n, k, options):
        blk = cls(n, k, options)
        blk.rate = 1.0
        blk.differentiate([types.Byte])
        blk.initialize()
        return blk

    ccsds = {"gfpoly": 0x187, "fcr": 112, "prim": 11}
    for name, n, k, options in (("CCSDS (255,223) I=1", 255, 223, dict(ccsds)), ("CCSDS (255,223) I=5", 255, 223, dict(ccsds, interleave=5)),
                                ("DVB-S (204,188)", 204, 188, {})):
        I, t = options.get("interleave", 1), (n - k) // 2
        frames = -(-(1 << 24) // (I * k))
        message = torch.from_numpy(rng.integers(0, 256, frames * I * k).astype(np.uint8)).cuda()
        coded = torch.empty(frames * I * n, dtype=torch.uint8, device="cuda")
        enc = make(lr.ReedSolomonEncoderBlock, n, k, options)
        assert enc.process_device(message.data_ptr(), len(message), coded.data_ptr(), len(coded)) == len(coded)
        torch.cuda.synchronize()
        words = coded.cpu().numpy().reshape(frames, n, I).transpose(0, 2, 1).reshape(frames * I, n)      # [codeword][byte]
        inputs = [("encoder", enc, message, len(coded))]
        for label, share in (("decoder, clean", 0.0), ("decoder, t errors in 1 of 100", 0.01), ("decoder, t errors in every codeword", 1.0)):
            hit = words.copy()
            rows = np.arange(len(hit)) if share == 1.0 else np.flatnonzero(rng.random(len(hit)) < share)
            where = np.argsort(rng.random((len(rows), n)), axis=1)[:, :t]                                # t distinct positions per codeword
            hit[rows[:, None], where] ^= rng.integers(1, 256, where.shape).astype(np.uint8)
            x = torch.from_numpy(np.ascontiguousarray(hit.reshape(frames, I, n).transpose(0, 2, 1)).reshape(-1)).cuda()
            inputs.append((label, make(lr.ReedSolomonDecoderBlock, n, k, dict(options, status=True)), x, frames * I * (k + 1)))
        for label, blk, x, n_out in inputs:
            y = torch.empty(n_out + 64, dtype=torch.uint8, device="cuda")
            half = (len(x) + n_out) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            ms, ms_copy = [], []
            for _ in range(3):
                blk.reset()
                assert blk.process_device(x.data_ptr(), len(x), y.data_ptr(), n_out) == n_out
                ms.append(timed(lambda: blk.process_device(x.data_ptr(), len(x), y.data_ptr(), n_out)))
                ms_copy.append(timed(lambda: dst.copy_(src)))
            row = {"row": "ReedSolomon %s %s" % (name, label), "message_bytes": frames * I * k, "codewords": frames * I, "op": blk.op(), "ms": ms,
                   "copy_ms": ms_copy, "copy_bytes_moved": 2 * half, "share_of_copy": round(min(ms_copy) / min(ms), 3),
                   "GB/s_message": round(frames * I * k / min(ms) / 1e6, 2)}
            if label != "encoder":
                status = y[:n_out].cpu().numpy().reshape(frames, I * (k + 1))[:, I * k:]
                row["codewords_corrected"] = int(np.count_nonzero((status > 0) & (status <= t)))
                row["codewords_uncorrectable"] = int(np.count_nonzero(status == 255))
            line = json.dumps(row)
            print(line)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


def fecglue_rows(args):
    """PunctureBlock and DepunctureBlock at rate 3/4, the (12, 17) and (52, 4) interleavers, the 1504-byte scrambler and the DVB-S chains
    dvbs_fec_encoder / dvbs_fec_decoder at 3/4 end to end, on resident vectors of about 2^24 input bytes per call, successive calls continuing one
    stream.  Each row stands next to a device-to-device copy that moves the row's input plus output bytes (a buffer of half that size copied
    once), the two alternating three times.  The four stages are pure data movement, so share_of_copy is their figure; the chains are a record.
    --out appends the rows to a file (profiles/fec_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(3)

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    def made(blk, in_type):
        blk.rate = 1.0
        blk.differentiate([in_type])
        blk.initialize()
        return blk

    pattern = lr.DVBS_PUNCTURE["3/4"]
    n = 1 << 24
    packets = n // 188
    ts = rng.integers(0, 256, (packets, 188)).astype(np.uint8)
    ts[:, 0] = 0x47
    rows = [("Puncture 3/4", made(lr.PunctureBlock(pattern), types.Bit), rng.integers(0, 2, n // 6 * 6).astype(np.uint8)),
            ("Depuncture 3/4 (Float32 LLRs)", made(lr.DepunctureBlock(pattern), types.Float32), rng.standard_normal(n // 16 * 4).astype(np.float32)),
            ("ConvolutionalInterleaver (12,17)", made(lr.ConvolutionalInterleaverBlock(12, 17), types.Byte), rng.integers(0, 256, n).astype(np.uint8)),
            ("ConvolutionalDeinterleaver (12,17)", made(lr.ConvolutionalDeinterleaverBlock(12, 17), types.Byte), rng.integers(0, 256, n).astype(np.uint8)),
            ("ConvolutionalInterleaver (52,4)", made(lr.ConvolutionalInterleaverBlock(52, 4), types.Byte), rng.integers(0, 256, n).astype(np.uint8)),
            ("AdditiveScrambler DVB 1504-byte table", made(lr.AdditiveScramblerBlock(lr.dvb_energy_dispersal_table()), types.Byte),
             rng.integers(0, 256, n).astype(np.uint8)),
            ("dvbs_fec_encoder 3/4", lr.dvbs_fec_encoder("3/4"), ts.ravel()),
            ("dvbs_fec_decoder 3/4 (Float32 LLRs)", lr.dvbs_fec_decoder("3/4"), (4.0 * rng.standard_normal(n // 16 * 4)).astype(np.float32))]
    for label, obj, host in rows:
        x = torch.from_numpy(host).cuda()
        cap = obj.max_output(len(x))
        out_size = obj.out_type.dtype.itemsize if isinstance(obj, lr.Chain) else obj.get_output_type().dtype.itemsize
        y = torch.empty(cap * out_size + 64, dtype=torch.uint8, device="cuda")
        in_bytes = len(x) * host.dtype.itemsize
        ms, ms_copy, counts = [], [], []
        for _ in range(3):
            obj.reset()
            counts = [obj.process_device(x.data_ptr(), len(x), y.data_ptr(), cap) for _ in range(2)]      # the second call is the steady state
            half = (in_bytes + counts[1] * out_size) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            ms.append(timed(lambda: obj.process_device(x.data_ptr(), len(x), y.data_ptr(), cap)))
            ms_copy.append(timed(lambda: dst.copy_(src)))
        row = {"row": "FEC glue %s" % label, "input_bytes": in_bytes, "output_bytes": counts[1] * out_size, "ms": ms, "copy_ms": ms_copy,
               "copy_bytes_moved": 2 * half, "share_of_copy": round(min(ms_copy) / min(ms), 3), "GB/s_input": round(in_bytes / min(ms) / 1e6, 2)}
        if isinstance(obj, lr.Chain):
            row["launches"] = obj.last_launches
        else:
            row["op"] = obj.op()[:80]
        line = json.dumps(row)
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


def ert_framer_rows(args):
    """The three ERT framers (kernels_ertframer.h) on 2^log2-samples resident Bit bytes - random bits with a valid frame (the encoders of
    tests/helpers/ert_framer_model.py) planted every 4 L bits - each next to a read-only pass over the same bytes (torch's sum: a yardstick for
    the load stream, not one of the library's kernels), the two alternating three times.  A call includes the framer's one count read-back.
    A record, not an acceptance criterion.  --out appends the rows to a file (profiles/ert_framer_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types
    from tests.helpers import ert_framer_model as M

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(1)
    n = 1 << args.log2_samples

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    for name, cls in (("scm", lr.SCMFramerBlock), ("scm+", lr.SCMPlusFramerBlock), ("idm", lr.IDMFramerBlock)):
        P = M.PROTOCOLS[name]
        bits = rng.integers(0, 2, n).astype(np.uint8)
        frames = [M.random_frame(P, rng)[0] for _ in range(16)]
        planted = 0
        for at in range(P.L, n - P.L, 4 * P.L):
            bits[at:at + P.L] = frames[planted % len(frames)]
            planted += 1
        x = torch.from_numpy(bits).cuda()
        blk = cls()
        blk.rate = 16384.0
        blk.differentiate([types.Bit])
        blk.initialize()
        cap = blk.max_output(n)
        y = torch.empty(cap * P.dtype.itemsize + 64, dtype=torch.uint8, device="cuda")
        count = []

        def call():                                   # successive calls continue one stream (the carried bytes of the call before)
            count.append(blk.process_device(x.data_ptr(), n, y.data_ptr(), cap))
        ms, ms_read = [], []
        for _ in range(3):
            ms.append(timed(call))
            ms_read.append(timed(lambda: x.sum()))
        row = {"row": "%s L=%d" % (cls.name, P.L), "bits": n, "frames_planted": planted, "frames_found": int(count[-1]), "ms": ms,
               "read_only_ms": ms_read, "share_of_read_only": round(min(ms_read) / min(ms), 3), "Gbit/s": round(n / min(ms) / 1e6, 2)}
        line = json.dumps(row)
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


def packet_framer_rows(args):
    """AX25FramerBlock and POCSAGFramerBlock (kernels_ax25framer.h, kernels_pocsagframer.h) on 2^log2-samples resident Bit bytes, two inputs
    each: random bits, and back-to-back frames (AX.25: flag, frame, flag with 0 .. 39 payload octets; POCSAG: batches of messages of 0 .. 6 data
    words, the builders of tests/helpers/ax25_model.py and pocsag_model.py) - each next to a read-only pass over the same bytes (torch's sum), the
    two alternating three times.  A call includes the framer's one count read-back.  A record, not an acceptance criterion.  --out appends the
    rows to a file (profiles/packet_framer_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types
    from tests.helpers import ax25_model as A
    from tests.helpers import pocsag_model as P

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(1)
    n = 1 << args.log2_samples

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    def tiled(pieces):
        out = np.concatenate(pieces)
        return np.tile(out, -(-n // len(out)))[:n]
    inputs = {
        (lr.AX25FramerBlock, "frames"): tiled([A.framed(A.random_octets(rng)) for _ in range(64)]),
        (lr.POCSAGFramerBlock, "frames"): tiled([P.transmission(P.random_messages(rng, 40))[0]]),
    }
    for cls, frame_type in ((lr.AX25FramerBlock, types.AX25FrameType), (lr.POCSAGFramerBlock, types.POCSAGFrameType)):
        for kind in ("random", "frames"):
            bits = rng.integers(0, 2, n).astype(np.uint8) if kind == "random" else inputs[(cls, kind)]
            x = torch.from_numpy(bits).cuda()
            blk = cls()
            blk.rate = 1200.0
            blk.differentiate([types.Bit])
            blk.initialize()
            cap = blk.max_output(n)
            y = torch.empty(cap * frame_type.dtype.itemsize + 64, dtype=torch.uint8, device="cuda")
            count = []

            def call():                               # successive calls continue one stream (the carried bytes of the call before)
                count.append(blk.process_device(x.data_ptr(), n, y.data_ptr(), cap))
            ms, ms_read = [], []
            for _ in range(3):
                ms.append(timed(call))
                ms_read.append(timed(lambda: x.sum()))
            row = {"row": "%s %s" % (cls.name, kind), "bits": n, "records_found": int(count[-1]), "ms": ms, "read_only_ms": ms_read,
                   "share_of_read_only": round(min(ms_read) / min(ms), 3), "Gbit/s": round(n / min(ms) / 1e6, 2)}
            line = json.dumps(row)
            print(line)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


def varicode_rows(args):
    """VaricodeDecoderBlock (kernels_varicode.h) on 2^log2-samples resident Bit bytes (--log2-samples 24 for the recorded rows), two inputs:
    random bits, and an encoded text (random characters with codes of at most 8 bits, the encoder of tests/helpers/varicode_model.py, tiled) -
    each next to a read-only pass over the same bytes (torch's sum), the two alternating three times.  A call includes the decoder's one count
    read-back.  A record, not an acceptance criterion: 31.25 bit/s is no hot path.  --out appends the rows to a file
    (profiles/varicode_table.jsonl)."""
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types
    from tests.helpers import varicode_model as V

    lr.init(0)
    lr.adopt_torch_stream()
    rng = np.random.default_rng(1)
    n = 1 << args.log2_samples

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
        return round(e0.elapsed_time(e1) / args.reps, 4)

    short = [c for c in range(128) if V.CODE[c] < 0x100]
    text = V.encode(rng.choice(short, 1 << 14).tolist())
    for kind in ("random", "text"):
        bits = rng.integers(0, 2, n).astype(np.uint8) if kind == "random" else np.tile(text, -(-n // len(text)))[:n]
        x = torch.from_numpy(bits).cuda()
        blk = lr.VaricodeDecoderBlock()
        blk.rate = 31.25
        blk.differentiate([types.Bit])
        blk.initialize()
        cap = blk.max_output(n)
        y = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
        count = []

        def call():                                   # successive calls continue one stream (the carried state of the call before)
            count.append(blk.process_device(x.data_ptr(), n, y.data_ptr(), cap))
        ms, ms_read = [], []
        for _ in range(3):
            ms.append(timed(call))
            ms_read.append(timed(lambda: x.sum()))
        row = {"row": "VaricodeDecoderBlock %s" % kind, "bits": n, "characters": int(count[-1]), "ms": ms, "read_only_ms": ms_read,
               "share_of_read_only": round(min(ms_read) / min(ms), 3), "Gbit/s": round(n / min(ms) / 1e6, 2)}
        line = json.dumps(row)
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
