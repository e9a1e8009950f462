#!/usr/bin/env python3
"""Per-block throughput table on one MI355X (the reference's benchmark suite is per block:
benchmarks/luaradio_benchmark.lua).  Device-resident vectors, HIP-event timing on the launch stream.
Prints one JSON object per block: MS/s (input samples), algorithmic GB/s, fraction of 8 TB/s, and the same
for the cheapest streaming kernel (MultiplyConstant) as the achievable-bandwidth yardstick."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated substrings: run only the rows whose name contains one of them")
    args = ap.parse_args()
    only = [t for t in args.only.split(",") if t]
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import spectrum_utils, types

    lr.init(0)
    L = lr._lib.load()
    lr.adopt_torch_stream()
    n = 1 << args.log2_samples
    g = torch.Generator(device="cuda").manual_seed(1)
    xc = torch.rand(2 * n, device="cuda", generator=g) * 2 - 1
    xr = xc[:n]
    out = torch.empty(2 * n + 64, device="cuda")

    def timeit(fn, reps=args.reps):
        fn()
        torch.cuda.synchronize()
        t = L.lrhip_timer_create()
        L.lrhip_timer_start(t)
        for _ in range(reps):
            fn()
        L.lrhip_timer_stop(t)
        ms = L.lrhip_timer_elapsed_ms(t) / reps
        L.lrhip_timer_destroy(t)
        return ms

    def mk(cls, args_, cplx, rate=1102500.0):
        b = cls(*args_)
        b.rate = rate
        b.differentiate([types.ComplexFloat32 if cplx else types.Float32])
        b.initialize()
        return b

    rows = []

    def run(name, blk, cplx, alg_bytes_per_sample, flops=0.0):
        if only and not any(t in name for t in only):
            return
        blk = blk()
        x = xc if cplx else xr
        cap = blk.max_output(n)
        dst = out if cap * (2 if cplx else 1) <= out.numel() else torch.empty(cap * 2 + 64, device="cuda")
        ms = timeit(lambda: blk.process_device(x.data_ptr(), n, dst.data_ptr(), cap))
        gbs = alg_bytes_per_sample * n / ms / 1e6
        rows.append({"block": name, "MS/s": round(n / ms / 1e3, 1), "alg_GB/s": round(gbs, 1), "frac_8TB/s": round(gbs / 8000, 4),
                     "ms": round(ms, 4), "TFLOP/s": round(flops * n / ms / 1e9, 2) if flops else None})

    taps128 = lr.filter_utils.firwin_lowpass(128, 15e3 / 110250)
    # yardstick: the cheapest streaming kernel (one multiply per scalar), 8 B in + 8 B out per sample
    run("MultiplyConstant(1.0) cf32 (streaming yardstick)", lambda: mk(lr.MultiplyConstantBlock, [1.0], True), True, 16)
    run("FIRFilter 128 real taps, cf32, direct form (use_fft=False)", lambda: mk(lr.FIRFilterBlock, [taps128, False], True), True, 16, 512)
    run("FIRFilter 128 real taps, cf32, overlap-save (use_fft=fast)", lambda: mk(lr.FIRFilterBlock, [taps128, "fast"], True), True, 16, 125)
    run("FIRFilter 128 real taps, f32, direct form (use_fft=False)", lambda: mk(lr.FIRFilterBlock, [taps128, False], False), False, 8, 256)
    run("FIRFilter 128 real taps, f32, overlap-save (use_fft=fast)", lambda: mk(lr.FIRFilterBlock, [taps128, "fast"], False), False, 8, 63)
    taps1276 = np.convolve(np.convolve(np.convolve(np.convolve(lr.filter_utils.firwin_lowpass(256, 0.3), lr.filter_utils.firwin_lowpass(256, 0.35)),
                                                   lr.filter_utils.firwin_lowpass(256, 0.4)), lr.filter_utils.firwin_lowpass(256, 0.45)),
                           lr.filter_utils.firwin_lowpass(256, 0.5)).astype(np.float32)
    run("FIRFilter 1276 real taps, cf32, overlap-save (4096-point blocks)", lambda: mk(lr.FIRFilterBlock, [taps1276, "fast"], True), True, 16, 180)
    run("FIRFilter 768 real taps, cf32, overlap-save (4096-point blocks)", lambda: mk(lr.FIRFilterBlock, [taps1276[:768], "fast"], True), True, 16, 160)
    # round 6: Float32 streams above 512 taps on the 64 x 64 kernel (round 4-5: the partitioned kernel of kernels_firpols.h, LRHIP_F64_F32=0)
    run("FIRFilter 1276 real taps, f32, overlap-save (64 x 64 kernel, two stream blocks per transform)", lambda: mk(lr.FIRFilterBlock, [taps1276, "fast"], False), False, 8, 250)
    taps4096 = np.resize(taps1276, 4096).astype(np.float32) / 4.0
    # (the 8 192-tap rows first: their two launches are the kernel of the 4 096-tap rows, whose dispatches must be the LAST ones of that kernel in the trace -
    # profiles/summarize_rocpd.py --last 10)
    run("FIRFilter 8192 real taps, cf32, overlap-save (four partitions of the 64 x 64 kernel, TWO launches)", lambda: mk(lr.FIRFilterBlock, [np.resize(taps1276, 8192).astype(np.float32) / 8.0, "fast"], True), True, 16, 1300)
    run("FIRFilter 8192 real taps, f32, overlap-save (four partitions of the 64 x 64 kernel, TWO launches)", lambda: mk(lr.FIRFilterBlock, [np.resize(taps1276, 8192).astype(np.float32) / 8.0, "fast"], False), False, 8, 650)
    run("FIRFilter 768 real taps, f32, overlap-save (64 x 64 kernel, two stream blocks per transform)", lambda: mk(lr.FIRFilterBlock, [taps1276[:768], "fast"], False), False, 8, 160)
    run("FIRFilter 2048 real taps, f32, overlap-save (64 x 64 kernel at an overlap of 2 048)", lambda: mk(lr.FIRFilterBlock, [taps4096[:2048], "fast"], False), False, 8, 240)
    run("FIRFilter 4096 real taps, f32, overlap-save (two partitions of the 64 x 64 kernel, ONE launch)", lambda: mk(lr.FIRFilterBlock, [taps4096, "fast"], False), False, 8, 420)
    run("FIRFilter 4096 real taps, cf32, overlap-save (two partitions of the 64 x 64 kernel, ONE launch)", lambda: mk(lr.FIRFilterBlock, [taps4096, "fast"], True), True, 16, 420)
    run("FIRFilter 2048 real taps, cf32, overlap-save (64 x 64 kernel at an overlap of 2 048)", lambda: mk(lr.FIRFilterBlock, [taps4096[:2048], "fast"], True), True, 16, 240)
    run("FIRFilter 1276 complex taps, cf32, overlap-save (4096-point blocks, four waves per CU)",
        lambda: mk(lr.FIRFilterBlock, [np.asarray(taps1276, np.complex64) * (1 + 0.5j), "fast"], True), True, 16, 180)
    run("FIRFilter 16 real taps, cf32", lambda: mk(lr.FIRFilterBlock, [taps128[:16], False], True), True, 16, 64)
    run("FIRFilter 128 complex taps, cf32, direct form (use_fft=False)", lambda: mk(lr.FIRFilterBlock, [np.asarray(taps128, np.complex64) * (1 + 0.5j), False], True), True, 16, 1024)
    run("FIRFilter 128 complex taps, cf32, overlap-save (use_fft=fast)", lambda: mk(lr.FIRFilterBlock, [np.asarray(taps128, np.complex64) * (1 + 0.5j), "fast"], True), True, 16, 125)
    run("FrequencyTranslator", lambda: mk(lr.FrequencyTranslatorBlock, [-250e3], True), True, 16)
    run("FrequencyDiscriminator", lambda: mk(lr.FrequencyDiscriminatorBlock, [1.25], True), True, 12)
    run("Downsampler(5) cf32", lambda: mk(lr.DownsamplerBlock, [5], True), True, 8 + 8 / 5)
    run("Downsampler(5) f32", lambda: mk(lr.DownsamplerBlock, [5], False), False, 4 + 4 / 5)
    run("FMDeemphasis f32", lambda: mk(lr.FMDeemphasisFilterBlock, [75e-6], False, 220500.0), False, 8)
    run("Decimator(5) cf32 (fused FIR+downsample)", lambda: mk(lr.DecimatorBlock, [5, {"use_fft": False}], True), True, 8 + 8 / 5, 4 * 128 / 5)
    run("Tuner(-250k,200k,5) (fused rot+FIR+downsample)", lambda: mk(lr.TunerBlock, [-250e3, 200e3, 5, {"use_fft": False}], True), True, 8 + 8 / 5, 4 * 128 / 5 + 6)
    run("Tuner(-100k,10k,50) (the AM / SSB / NBFM receivers' tuner: LDS-staged decimator)", lambda: mk(lr.TunerBlock, [-100e3, 10e3, 50, {"use_fft": False}], True), True, 8 + 8 / 50, 4 * 128 / 50 + 6)
    run("Tuner(-100k,12k,80) (rtlsdr_pocsag.lua / rtlsdr_ax25.lua: LDS-staged decimator, phase-array layout)", lambda: mk(lr.TunerBlock, [-100e3, 12e3, 80, {"use_fft": False}], True), True, 8 + 8 / 80, 4 * 128 / 80 + 6)
    run("Decimator(25) cf32 (LDS-staged decimator, no rotator)", lambda: mk(lr.DecimatorBlock, [25, {"use_fft": False}], True), True, 8 + 8 / 25, 4 * 128 / 25)
    run("Decimator(5) cf32, polyphase FFT overlap-save", lambda: mk(lr.DecimatorBlock, [5, {"use_fft": "fast"}], True), True, 8 + 8 / 5, 62)
    run("Tuner(-250k,200k,5), polyphase FFT overlap-save", lambda: mk(lr.TunerBlock, [-250e3, 200e3, 5, {"use_fft": "fast"}], True), True, 8 + 8 / 5, 62)
    # write-heavy yardstick: the zero-stuffing Upsampler moves exactly the Interpolator's bytes (8 B in, 8 L B out per input sample) with no arithmetic
    run("Upsampler(5) cf32 (the Interpolator's traffic without arithmetic: write-heavy yardstick)", lambda: mk(lr.UpsamplerBlock, [5], True), True, 8 + 8 * 5)
    run("Interpolator(5) cf32 (polyphase, input samples)", lambda: mk(lr.InterpolatorBlock, [5], True), True, 8 + 8 * 5, 4 * 128)
    run("RationalResampler(3, 2) cf32 (polyphase, input samples)", lambda: mk(lr.RationalResamplerBlock, [3, 2], True), True, 8 + 8 * 1.5, 4 * 128 * 1.5 / 3)
    run("RationalResampler(2, 3) cf32 (polyphase, input samples)", lambda: mk(lr.RationalResamplerBlock, [2, 3], True), True, 8 + 8 * 2 / 3, 4 * 128 * (2 / 3) / 2)
    run("RationalResampler(4, 3) cf32 (polyphase, input samples)", lambda: mk(lr.RationalResamplerBlock, [4, 3], True), True, 8 + 8 * 4 / 3, 4 * 128 * (4 / 3) / 4)
    run("RationalResampler(5, 4) cf32 (polyphase, input samples)", lambda: mk(lr.RationalResamplerBlock, [5, 4], True), True, 8 + 8 * 5 / 4, 4 * 128 * (5 / 4) / 5)
    run("RationalResampler(3, 4) cf32 (polyphase, input samples)", lambda: mk(lr.RationalResamplerBlock, [3, 4], True), True, 8 + 8 * 3 / 4, 4 * 128 * (3 / 4) / 3)
    run("RationalResampler(4, 5) cf32 (polyphase, input samples)", lambda: mk(lr.RationalResamplerBlock, [4, 5], True), True, 8 + 8 * 4 / 5, 4 * 128 * (4 / 5) / 4)
    # IQFileSource's sample formats converted on the device (iqfile.lua:82-116, format_utils.lua:82-97): raw records in, ComplexFloat32 out
    class _Fmt:
        def __init__(self, fmt):
            self.q = L.lrhip_format_convert_create(fmt.encode(), 1)
            assert self.q, lr._lib.last_error()

        def max_output(self, n_):
            return n_

        def process_device(self, xp, n_, yp, cap):
            return lr._lib.check(L.lrhip_stage_execute_device(self.q, xp, n_, yp, cap), "format")

    run("IQ records u8 -> cf32 (device)", lambda: _Fmt("u8"), True, 2 + 8)
    run("IQ records s16le -> cf32 (device)", lambda: _Fmt("s16le"), True, 4 + 8)
    run("IQ records f32be -> cf32 (device)", lambda: _Fmt("f32be"), True, 8 + 8)
    run("HilbertTransform(65) f32 -> cf32", lambda: mk(lr.HilbertTransformBlock, [65], False), False, 12, 2 * 65)
    run("HilbertTransform(129) f32 -> cf32", lambda: mk(lr.HilbertTransformBlock, [129], False), False, 12, 2 * 129)
    # the reference suite's IIR entry (benchmarks/luaradio_benchmark.lua: 5 feed-forward, 3 feedback taps), a stable filter
    b_iir, a_iir = [0.0976, 0.1953, 0.0976, 0.05, 0.02], [1.0, -0.9428, 0.3333]
    run("IIRFilter 5 ff / 3 fb cf32", lambda: mk(lr.IIRFilterBlock, [b_iir, a_iir], True), True, 16)
    run("IIRFilter 5 ff / 3 fb f32", lambda: mk(lr.IIRFilterBlock, [b_iir, a_iir], False), False, 8)
    run("IIRFilter 3 ff / 3 fb (biquad) cf32", lambda: mk(lr.IIRFilterBlock, [b_iir[:3], a_iir], True), True, 16)
    # the ERT receiver's sampler (kernels_preamble.h: match, walk, emit + one count read-back) at 393 216 S/s, 2^24 resident Float32 samples: on noise
    # (the match pass leaves its tap loop after a couple of taps, no frame) and with an SCM frame every 20 000 samples; next to it the clocksampler,
    # the other multi-pass stage with a read-back, on the same noise; then ert_receiver with all three protocols (a DeviceGraph: host vectors, the
    # copies in and out are part of its time)
    if not only or any(t in "PreambleSampler ClockSampler ert_receiver" for t in only):
        from luaradio_amd import composites as comp
        m = min(n, 1 << 24)
        rng = np.random.default_rng(2)
        framed = (0.1 * rng.standard_normal(m)).astype(np.float32)
        bits = np.concatenate([np.array(comp.SCM_PREAMBLE), rng.integers(0, 2, comp.SCM_FRAME_LEN - len(comp.SCM_PREAMBLE))])
        wave = np.repeat(np.where(bits > 0, 1.0, -1.0), 24) * np.tile(1.0 - 0.5 * np.abs(np.linspace(-1, 1, 24)), len(bits))
        for at in range(1000, m - len(wave), 20000):
            framed[at:at + len(wave)] = wave
        xf = torch.from_numpy(framed).cuda()
        for name, cls, a, x_ in (("PreambleSampler(16384, SCM_PREAMBLE, 96) @ 393216, noise", lr.PreambleSamplerBlock, [16384, comp.SCM_PREAMBLE, 96], xr[:m]),
                                 ("PreambleSampler(16384, SCM_PREAMBLE, 96) @ 393216, a frame every 20 000 samples", lr.PreambleSamplerBlock,
                                  [16384, comp.SCM_PREAMBLE, 96], xf),
                                 ("ClockSampler(16384) @ 393216, noise (yardstick: multi-pass stage with a count read-back)", lr.ClockSamplerBlock, [16384], xr[:m])):
            chn = lr.Chain([mk(cls, a, False, 393216.0)])
            cap = chn.max_output(m)
            got = []
            ms = timeit(lambda: got.append(chn.process_device(x_.data_ptr(), m, out.data_ptr(), cap)))
            rows.append({"block": name, "MS/s": round(m / ms / 1e3, 1), "alg_GB/s": round(4 * m / ms / 1e6, 1), "frac_8TB/s": round(4 * m / ms / 1e6 / 8000, 4),
                         "ms": round(ms, 4), "TFLOP/s": None, "samples": m, "outputs": int(got[-1]), "launches": chn.last_launches})
        gx = lr.ert_receiver(rate=2359296.0)
        xh = xc[:2 * m].cpu().numpy().view(np.complex64)
        ms = timeit(lambda: gx.process(**{"in": xh}), reps=3)
        rows.append({"block": "ert_receiver(idm, scm, scm+) @ 2359296 (host vectors: copies in and out included)", "MS/s": round(m / ms / 1e3, 1), "ms": round(ms, 4),
                     "samples": m, "launches": sum(nd.runner.last_launches for nd in gx._order if nd.runner is not None)})
    # the generator sources (kernels_source.h): write-only kernels, 8 / 4 / 1 bytes per sample and no read at all.  They alternate with the streaming
    # yardstick (MultiplyConstant cf32, 8 B in + 8 B out per sample) on the same output buffer; the figure of merit is bytes moved per second over the
    # yardstick's in the same runs, every run listed
    if not only or any(t in "SignalSource UniformRandomSource" for t in only):
        def source(blk):
            blk.initialize()
            return blk

        mcs = mk(lr.MultiplyConstantBlock, [1.0], True)
        cases = [("SignalSource exponential cf32", source(lr.SignalSource("exponential", 250e3, 2e6)), 8),
                 ("SignalSource cosine f32", source(lr.SignalSource("cosine", 100e3, 1e6, {"amplitude": 2.5})), 4),
                 ("SignalSource square f32", source(lr.SignalSource("square", 1e3, 2e6, {"offset": 1.0})), 4),
                 ("UniformRandomSource cf32", source(lr.UniformRandomSource(types.ComplexFloat32, 1e6)), 8),
                 ("UniformRandomSource f32", source(lr.UniformRandomSource(types.Float32, 1e6)), 4),
                 ("UniformRandomSource bit", source(lr.UniformRandomSource(types.Bit, 1e3)), 1)]
        runs = {name: [] for name, _, _ in cases}
        runs["stream"] = []
        for _ in range(4):
            runs["stream"].append(timeit(lambda: mcs.process_device(xc.data_ptr(), n, out.data_ptr(), n)))
            for name, src, _ in cases:
                runs[name].append(timeit(lambda: src.process_device(out.data_ptr(), n)))
        stream = sorted(runs["stream"])[len(runs["stream"]) // 2]
        for name, key, bps in [("MultiplyConstant(1.0) cf32 (streaming yardstick, alternating with the sources)", "stream", 16)] + [(c[0], c[0], c[2]) for c in cases]:
            ms_ = sorted(runs[key])[len(runs[key]) // 2]
            rows.append({"block": name, "MS/s": round(n / ms_ / 1e3, 1), "bytes_per_sample": bps, "alg_GB/s": round(bps * n / ms_ / 1e6, 1),
                         "frac_8TB/s": round(bps * n / ms_ / 1e6 / 8000, 4), "ms": round(ms_, 4), "ms_runs": [round(v, 4) for v in runs[key]],
                         "bytes_per_s_over_streaming_yardstick": round((bps / ms_) / (16 / stream), 3)})
    # the synthesis filterbank (kernels_pfbsynth.h): 2^24 frame values in (8 B each) and 2^24 / R samples out per call.  The synthesis block, the analysis
    # block of the same shape (2^24 samples in, R 2^24 values out) and the streaming yardstick alternate on the same buffers, five runs of 10 calls; the
    # figure of merit is bytes moved per second over the yardstick's (16 B per sample) in the same runs, every run listed
    if not only or any(t in "PolyphaseSynthesizer" for t in only):
        ns = min(n, 1 << 24)
        mcy = mk(lr.MultiplyConstantBlock, [1.0], True)
        for k_, m_ in ((64, 1024), (1024, 16384)):
            taps_ = lr.filter_utils.firwin_lowpass(m_, 1.0 / k_)
            for r_ in (1, 2, 4):
                syn = mk(lr.PolyphaseSynthesizerBlock, [k_, taps_, {"oversample": r_}], True)
                ana = mk(lr.PolyphaseChannelizerBlock, [k_, taps_, {"method": "fft", "oversample": r_}], True)
                cap_s = max(ana.max_output(ns), syn.max_output(ns), ns)
                big_s = torch.empty(2 * cap_s + 64, device="cuda")
                runs = {"syn": [], "ana": [], "stream": []}
                for _ in range(5):
                    runs["syn"].append(timeit(lambda: syn.process_device(xc.data_ptr(), ns, big_s.data_ptr(), cap_s), reps=10))
                    runs["ana"].append(timeit(lambda: ana.process_device(xc.data_ptr(), ns, big_s.data_ptr(), cap_s), reps=10))
                    runs["stream"].append(timeit(lambda: mcy.process_device(xc.data_ptr(), ns, big_s.data_ptr(), cap_s), reps=10))
                stream_ms = sorted(runs["stream"])[2]
                for name, key, bps in (("MultiplyConstant(1.0) cf32 (streaming yardstick, alternating with the synthesizer K=%d R=%d)" % (k_, r_), "stream", 16.0),
                                       ("PolyphaseChannelizer K=%d, %d taps, oversample=%d (analysis, alternating with the synthesizer)" % (k_, m_, r_), "ana", 8.0 * (1 + r_)),
                                       ("PolyphaseSynthesizer K=%d, %d taps, oversample=%d (polyphase + FFT, two launches)" % (k_, m_, r_), "syn", 8.0 * (1 + 1.0 / r_))):
                    ms_ = sorted(runs[key])[2]
                    rows.append({"block": name, "values_in": ns, "bytes_per_value": bps, "ms": round(ms_, 4), "ms_min": round(min(runs[key]), 4),
                                 "ms_max": round(max(runs[key]), 4), "ms_runs": [round(v, 4) for v in runs[key]], "alg_GB/s": round(bps * ns / ms_ / 1e6, 1),
                                 "bytes_per_s_over_streaming_yardstick": round((bps / ms_) / (16 / stream_ms), 3)})
                del big_s
    if only and not any(t in "WBFM PSD Channelizer" for t in only):
        for r in rows:
            print(json.dumps(r))
        return
    rx0 = lr.wbfm_mono_receiver(1102500.0, -250e3, use_fft=False)
    cap = rx0.max_output(n)
    ms = timeit(lambda: rx0.process_device(xc.data_ptr(), n, out.data_ptr(), cap))
    rows.append({"block": "WBFM mono chain, direct-form tuner (RF samples in)", "MS/s": round(n / ms / 1e3, 1), "alg_GB/s": round(8.16 * n / ms / 1e6, 1),
                 "frac_8TB/s": round(8.16 * n / ms / 1e6 / 8000, 4), "ms": round(ms, 4), "TFLOP/s": None, "launches": rx0.chain.last_launches})
    rx = lr.wbfm_mono_receiver(1102500.0, -250e3)
    cap = rx.max_output(n)
    ms = timeit(lambda: rx.process_device(xc.data_ptr(), n, out.data_ptr(), cap))
    rows.append({"block": "WBFM mono chain (RF samples in)", "MS/s": round(n / ms / 1e3, 1), "alg_GB/s": round(8.16 * n / ms / 1e6, 1),
                 "frac_8TB/s": round(8.16 * n / ms / 1e6 / 8000, 4), "ms": round(ms, 4), "TFLOP/s": None, "launches": rx.chain.last_launches})
    # a fan-out branch fed from an IQ file: [format stage (u8 records), Tuner(-350e3, 100e3, 5)] - one launch of the persistent Toeplitz kernel on the records
    def tuner_chain(head, decim=5):
        blocks = head + [lr.FrequencyTranslatorBlock(-350e3), lr.LowpassFilterBlock(128, 500e3 / decim), lr.DownsamplerBlock(decim)]
        r, t = 1102500.0, types.ComplexFloat32
        for b in blocks[len(head):]:
            b.rate = r
            b.differentiate([t])
            b.initialize()
            r, t = b.get_rate(), b.get_output_type()
        return lr.Chain(blocks)

    if True:
        src8 = lr.IQFileSource(bytes(16), "u8", 1102500.0)
        src8.initialize()
        tch = tuner_chain([src8])
        raw8t = (torch.rand(2 * n + 64, device="cuda") * 256).to(torch.uint8)
        capt = tch.max_output(n)
        ms = timeit(lambda: tch.process_device(raw8t.data_ptr(), n, out.data_ptr(), capt))
        src50 = lr.IQFileSource(bytes(16), "u8", 1102500.0)
        src50.initialize()
        tch50 = tuner_chain([src50], 50)
        cap50 = tch50.max_output(n)
        ms50 = timeit(lambda: tch50.process_device(raw8t.data_ptr(), n, out.data_ptr(), cap50))
        rows.append({"block": "Tuner(decimation 50) from u8 IQ records (AM / SSB / NBFM receivers fed from a file)", "MS/s": round(n / ms50 / 1e3, 1),
                     "alg_GB/s": round(2.16 * n / ms50 / 1e6, 1), "frac_8TB/s": round(2.16 * n / ms50 / 1e6 / 8000, 4), "ms": round(ms50, 4), "TFLOP/s": None,
                     "launches": tch50.last_launches})
        rows.append({"block": "Tuner from u8 IQ records (fan-out branch fed from a file)", "MS/s": round(n / ms / 1e3, 1), "alg_GB/s": round(3.6 * n / ms / 1e6, 1),
                     "frac_8TB/s": round(3.6 * n / ms / 1e6 / 8000, 4), "ms": round(ms, 4), "TFLOP/s": None, "launches": tch.last_launches})
    # the same receiver fed the raw unsigned 8-bit records of an RTL-SDR style IQ file (IQFileSource's format stage at the head of the chain): the single
    # launch reads the records itself; LRHIP_RX_NO_U8_FOLD=1 = conversion launch + receiver
    import importlib.util
    spec = importlib.util.spec_from_file_location("iqfile_wbfm_mono", os.path.join(ROOT, "examples", "iqfile_wbfm_mono.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    _src, ch8, _rate = ex.build_chain(bytes(16), "u8", 1102500.0, -250e3)
    raw8 = (torch.rand(2 * n + 64, device="cuda") * 256).to(torch.uint8)
    cap = ch8.max_output(n)
    ms = timeit(lambda: ch8.process_device(raw8.data_ptr(), n, out.data_ptr(), cap))
    rows.append({"block": "WBFM mono chain from u8 IQ records (RF samples in)", "MS/s": round(n / ms / 1e3, 1), "alg_GB/s": round(2.16 * n / ms / 1e6, 1),
                 "frac_8TB/s": round(2.16 * n / ms / 1e6 / 8000, 4), "ms": round(ms, 4), "TFLOP/s": None, "launches": ch8.last_launches})
    # PSD: frames of 1024
    N = 1024
    frames = n // N
    win = np.asarray(lr.window_utils.window(N, "hamming", True), np.float32)
    import ctypes as C
    st = L.lrhip_psd_create(N, win.ctypes.data_as(C.POINTER(C.c_float)), 1102500.0 * float(np.sum(win.astype(np.float64) ** 2)), 1, 1, 1)
    ms = timeit(lambda: L.lrhip_stage_execute_device(st, xc.data_ptr(), frames * N, out.data_ptr(), frames * N))
    rows.append({"block": "PSD N=1024 hamming log fftshift", "MS/s": round(n / ms / 1e3, 1), "alg_GB/s": round(12 * n / ms / 1e6, 1),
                 "frac_8TB/s": round(12 * n / ms / 1e6 / 8000, 4), "ms": round(ms, 4), "TFLOP/s": None})
    L.lrhip_stage_destroy(st)
    # configs[4]: 64-channel filterbank, 1024-tap prototype, as a dense GEMM on the f32 matrix cores
    ch = mk(lr.PolyphaseChannelizerBlock, [64], True)
    nch = min(n, 1 << 24)
    cap = ch.max_output(nch)
    big = torch.empty(2 * cap + 64, device="cuda")
    ms = timeit(lambda: ch.process_device(xc.data_ptr(), nch, big.data_ptr(), cap), reps=3)
    tf = 8.0 * 1024 * nch / ms / 1e9
    rows.append({"block": "PolyphaseChannelizer K=64, 1024 taps (dense MFMA GEMM)", "MS/s": round(nch / ms / 1e3, 1),
                 "alg_GB/s": round(16 * nch / ms / 1e6, 1), "frac_8TB/s": round(16 * nch / ms / 1e6 / 8000, 4), "ms": round(ms, 4),
                 "TFLOP/s": round(tf, 2), "mfma_util_vs_157.3TF": round(tf / 157.3, 4)})
    # the same filterbank in its polyphase + FFT form (method = "fft"), head to head: same process, same buffers, the GEMM, the FFT form and the streaming
    # yardstick (MultiplyConstant cf32, 16 B per sample like this block) alternating; every run listed, so the spread is on the row
    xs = torch.rand(2 * nch, device="cuda", generator=g) * 2 - 1        # uniform(-1, 1) like xc, but separate from the buffers of the rows above
    pfb = mk(lr.PolyphaseChannelizerBlock, [64, None, {"method": "fft"}], True)
    mc = mk(lr.MultiplyConstantBlock, [1.0], True)
    runs = {"gemm": [], "fft": [], "stream": []}
    for _ in range(4):
        runs["gemm"].append(timeit(lambda: ch.process_device(xs.data_ptr(), nch, big.data_ptr(), cap), reps=3))
        runs["fft"].append(timeit(lambda: pfb.process_device(xs.data_ptr(), nch, big.data_ptr(), cap), reps=10))
        runs["stream"].append(timeit(lambda: mc.process_device(xs.data_ptr(), nch, big.data_ptr(), cap), reps=10))
    stream_ms = sorted(runs["stream"])[len(runs["stream"]) // 2]

    def median(v):
        return sorted(v)[len(v) // 2]

    def pfb_row(name, ms_runs, extra):
        ms_ = median(ms_runs)
        row = {"block": name, "MS/s": round(nch / ms_ / 1e3, 1), "alg_GB/s": round(16 * nch / ms_ / 1e6, 1), "frac_8TB/s": round(16 * nch / ms_ / 1e6 / 8000, 4),
               "ms": round(ms_, 4), "ms_runs": [round(v, 4) for v in ms_runs], "frac_of_streaming_yardstick": round(stream_ms / ms_, 3)}
        row.update(extra)
        rows.append(row)

    pfb_row("MultiplyConstant(1.0) cf32 on the channelizer's buffers (streaming yardstick, alternating)", runs["stream"], {})
    pfb_row("PolyphaseChannelizer K=64, 1024 taps (dense MFMA GEMM, alternating)", runs["gemm"], {})
    pfb_row("PolyphaseChannelizer K=64, 1024 taps (polyphase + FFT)", runs["fft"],
            {"speedup_vs_gemm": round(median(runs["gemm"]) / median(runs["fft"]), 2), "gemm_spread_ms": round(max(runs["gemm"]) - min(runs["gemm"]), 4)})
    for k_, m_ in ((256, 4096), (1024, 16384), (4096, 65536)):
        blk = mk(lr.PolyphaseChannelizerBlock, [k_, lr.filter_utils.firwin_lowpass(m_, 1.0 / k_), {"method": "fft"}], True)
        pfb_row("PolyphaseChannelizer K=%d, %d taps (polyphase + FFT)" % (k_, m_),
                [timeit(lambda: blk.process_device(xs.data_ptr(), nch, big.data_ptr(), cap), reps=10) for _ in range(4)], {})
    # oversampled by R (hop K / R): 8 B in and 8 R B out per input sample.  The R = 1 block, the oversampled one and the streaming yardstick alternate on
    # the same buffers; the figure of merit is bytes moved per second over the yardstick's (16 B per sample) in the same runs
    for k_, m_ in ((64, 1024), (1024, 16384)):
        taps_ = lr.filter_utils.firwin_lowpass(m_, 1.0 / k_)
        crit = mk(lr.PolyphaseChannelizerBlock, [k_, taps_, {"method": "fft"}], True)
        for r_ in (2, 4):
            blk = mk(lr.PolyphaseChannelizerBlock, [k_, taps_, {"method": "fft", "oversample": r_}], True)
            cap_r = blk.max_output(nch)
            big_r = torch.empty(2 * cap_r + 64, device="cuda")
            runs = {"crit": [], "os": [], "stream": []}
            for _ in range(5):
                runs["crit"].append(timeit(lambda: crit.process_device(xs.data_ptr(), nch, big_r.data_ptr(), cap_r), reps=10))
                runs["os"].append(timeit(lambda: blk.process_device(xs.data_ptr(), nch, big_r.data_ptr(), cap_r), reps=10))
                runs["stream"].append(timeit(lambda: mc.process_device(xs.data_ptr(), nch, big_r.data_ptr(), cap_r), reps=10))
            for name, key, bps in (("MultiplyConstant(1.0) cf32 (streaming yardstick, alternating with K=%d R=%d)" % (k_, r_), "stream", 16),
                                   ("PolyphaseChannelizer K=%d, %d taps (polyphase + FFT, alternating with R=%d)" % (k_, m_, r_), "crit", 16),
                                   ("PolyphaseChannelizer K=%d, %d taps, oversample=%d (polyphase + FFT)" % (k_, m_, r_), "os", 8 * (1 + r_))):
                ms_ = median(runs[key])
                rows.append({"block": name, "MS/s": round(nch / ms_ / 1e3, 1), "bytes_per_sample": bps, "alg_GB/s": round(bps * nch / ms_ / 1e6, 1),
                             "frac_8TB/s": round(bps * nch / ms_ / 1e6 / 8000, 4), "ms": round(ms_, 4), "ms_runs": [round(v, 4) for v in runs[key]],
                             "bytes_per_s_over_streaming_yardstick": round((bps / ms_) / (16 / median(runs["stream"])), 3)})
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
