#!/usr/bin/env python3
"""bench.py - headline benchmark of the MI355X DSP block engine.

Contract: `python bench.py --gpus N --steps K --warmup W` prints ONE JSON line on rank 0.  With N > 1 and no launcher environment
(WORLD_SIZE / RANK unset) the script starts its own N ranks - it re-executes itself under `python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1` - the way the reference forks one process per block itself (radio/core/composite.lua:568-569);
launched by torchrun (the driver's form) it reads RANK / LOCAL_RANK / WORLD_SIZE from the environment and checks that WORLD_SIZE == --gpus.
A box with fewer than N devices makes it exit non-zero with a message (never a silent `"n_gpus": 1`), unless --same-device (dry runs).

Workloads (BASELINE.json configs):
  fir     (default; configs[1], the configuration the metric is quoted on) 128-tap real-taps FIR
          (LowpassFilterBlock(128, 15e3) at 220.5 kHz) on 2^28 synthetic ComplexFloat32 samples resident in
          HBM.  One step = one pass of FIRFilterBlock:process over the whole 2 GiB vector (one
          fir_mfma_kernel launch + the 1-block history-carry kernel).
  wbfm    (configs[2]) the examples/rtlsdr_wbfm_mono.lua chain, device-resident, on 2^26 RF samples.
  fanout  (configs[3]) one IQ slab broadcast from rank 0 to all ranks over RCCL, one Tuner branch per GPU.

N > 1: one process per GPU (self-launched or torchrun, see above), each rank filters its own independent stream of the same size
("scaling": "weak", no data-path collective for fir/wbfm); value = samples processed by all ranks / max time.

value = MSamples/s with inputs already in HBM.  roofline.achieved = algorithmic bytes (16 B/sample, SURVEY.md
section 8d) per launch / average launch duration measured with HIP events on the launch stream inside the timed region.
cpu_baseline = the reference's two CPU forms of the block (oracle/lr_cpu_baseline.c: FFT overlap-save = its default, and one
SIMD dot product per output) timed on this box's host cores on a bounded sample of the same workload, 5 trials, mean and
sigma (rank 0, N = 1 only).  verified / max_err = the output of the last timed step checked against the oracle on slabs.
At N = 1 the line also carries wbfm_chain (configs[2]), channelizer (configs[4]) and fanout (configs[3], degenerate) legs.
--dump-outputs DIR writes the output of the last timed step (inputs are seeded: the same arguments give the same arrays), so that two builds
can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: f32 vector == f32 MFMA peak
DUMP_BYTES = 48 << 20        # --dump-outputs: what all ranks write together


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="fir", choices=["fir", "wbfm", "fanout", "timeshard"])
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (and, for fanout, the RCCL broadcast) even with one rank: "
                                                              "exercises the N > 1 code path on a single GPU")
    ap.add_argument("--log2-samples", type=int, default=None, help="per-GPU samples per step (default 28 fir, 26 wbfm/fanout); timeshard: the WHOLE recording (default 28)")
    ap.add_argument("--fir-mode", default="auto", choices=["auto", "direct", "fft"],
                    help="fir workload arithmetic: direct = Toeplitz MFMA (bit-exact fmaf chain); fft = fused overlap-save kernel; "
                         "auto = fft (the faster one; both are parity-tested)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only for dry runs of the multi-rank plumbing)")
    ap.add_argument("--same-device", action="store_true", help="dry run: every rank uses cuda:0 (needs --dist-backend gloo)")
    ap.add_argument("--prewarm-ms", type=float, default=250.0, help="untimed clock-ramp period before the warm-up steps")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle check of the timed FIR output")
    ap.add_argument("--headline-only", action="store_true", help="fir workload: skip the wbfm_chain / channelizer / fanout legs of the line")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU baseline budget (seconds of CPU work)")
    ap.add_argument("--launch-check", action="store_true", help="every rank prints {rank, local_rank, world, gpus} and exits before touching a device: "
                                                                "the self-launch of --gpus N exercised on a box without GPUs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy in float32 (rank<r>_<name>.npy with N > 1); an output over its share "
                         "of %d MB is cut to a fixed, seeded sample of rows, whose positions go to DIR/<name>_index.npy in float64" % (DUMP_BYTES >> 20))
    return ap.parse_args()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 outside a launcher: start `torch.distributed.run` with N ranks of this same command line as a child and exit with its code
    (radio/core/composite.lua:568-569: the reference starts its own processes, the user never does).  Returns only if no launch is needed."""
    launched = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if launched:
        world = int(os.environ["WORLD_SIZE"])
        if world != args.gpus:
            raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
        return
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.gpus == 1:
        return
    if not args.launch_check:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus and not (args.same_device and have >= 1):
            raise SystemExit("bench.py: --gpus %d asked for, %d device(s) visible on this box - refusing to print a line for fewer GPUs than "
                             "requested (use --same-device --dist-backend gloo for a dry run of the multi-rank plumbing on one device)" % (args.gpus, have))
        if args.same_device and args.dist_backend == "nccl":
            raise SystemExit("bench.py: --same-device needs --dist-backend gloo (RCCL refuses two ranks on one device)")
    import subprocess
    sys.stdout.flush()
    sys.stderr.flush()
    # the launcher runs as a child (the ranks inherit stdout): a rendezvous that loses its port between _free_port() and the launcher's bind - the one
    # failure that is nobody's fault - is retried on a fresh port instead of failing the run
    for attempt in range(3):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        sys.stderr.write(r.stderr)
        sys.stderr.flush()
        # only the launcher's own bind failing counts (a generic DistNetworkError of a rank that died for another reason must not re-run the
        # bench and print a second JSON line)
        port_lost = any(t in r.stderr for t in ("Address already in use", "EADDRINUSE", "failed to bind"))
        if r.returncode == 0 or not port_lost:
            raise SystemExit(r.returncode)
        sys.stderr.write("bench.py: the rendezvous port was taken, launching again (attempt %d)\n" % (attempt + 2))
    raise SystemExit(r.returncode)


def _trials(fn, samples_per_call, seconds_per_trial, ntrials=5):
    """the reference suite's protocol (benchmarks/luaradio_benchmark.lua:10-13, :722-738): several trials, mean and sigma of
    samples/s; a trial repeats fn() until seconds_per_trial has elapsed"""
    import statistics
    fn()                                    # warm-up (page faults, OpenMP team start)
    rates = []
    for _ in range(ntrials):
        done, t0 = 0, time.perf_counter()
        while True:
            fn()
            done += samples_per_call
            dt = time.perf_counter() - t0
            if dt >= seconds_per_trial:
                break
        rates.append(done / dt / 1e6)
    return {"mean": round(statistics.mean(rates), 2), "sigma": round(statistics.pstdev(rates), 2), "trials": ntrials}


def cpu_baseline_fir(taps, budget_s):
    """The reference's two CPU forms of this block (oracle/lr_cpu_baseline.c), timed on this box's host cores on a bounded
    sample of the same workload (2^22-sample slabs of the same U(-1,1) IQ): (1) one SIMD dot product per output
    (firfilter.lua:129-145), (2) FFT overlap-save, the reference's default whenever FFTW is present (firfilter.lua:57,
    :320-398).  Each with one thread (the reference gives a block one core) and with the fastest OpenMP thread count;
    5 trials each, mean and sigma (luaradio_benchmark.lua:10-13)."""
    import numpy as np
    from oracle import oracle as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    n = 1 << 22
    rng = np.random.default_rng(2)
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    y = np.empty(n, np.complex64)
    forms = {"dot_product": O.baseline_fir_dot, "overlap_save": O.baseline_fir_overlap_save}
    per_trial = budget_s / 30.0             # 4 timed legs x 5 trials (+ probes) + the two half-length configs[0] legs
    out = {}
    for name, fn in forms.items():
        # pick the thread count that is actually fastest on this box (cgroup quotas make "all logical CPUs" a bad guess)
        cands = sorted({c for c in (2, 4, 8, 16, 32, 64, 128, avail) if c <= avail})
        probe = {}
        for c in cands:
            fn(taps, x[:1 << 18], c, out=y[:1 << 18])
            t0 = time.perf_counter()
            fn(taps, x, c, out=y)
            probe[c] = n / (time.perf_counter() - t0)
        cores = max(probe, key=probe.get)
        out[name] = {"single_core": _trials(lambda: fn(taps, x, 1, out=y), n, per_trial),
                     "all_cores": dict(_trials(lambda: fn(taps, x, cores, out=y), n, per_trial), threads=cores)}
    prod = out["overlap_save"]
    # BASELINE.json configs[0] as the reference's benchmark runs it: LowpassFilterBlock(128, ..) over 1 Mi ComplexFloat32 samples per pass, one core
    n0 = 1 << 20
    configs0 = {"samples_per_pass": n0, "single_core": {name: _trials(lambda fn=fn: fn(taps, x[:n0], 1, out=y[:n0]), n0, per_trial / 2.0) for name, fn in forms.items()}}
    return {"configs0": configs0, "slab_samples": n, "value": prod["all_cores"]["mean"], "sigma": prod["all_cores"]["sigma"], "unit": "MSamples/s", "cores": prod["all_cores"]["threads"],
            "kind": "port", "single_core_value": prod["single_core"]["mean"], "forms": out, "logical_cpus": avail,
            "sample": "oracle/lr_cpu_baseline.c on 2^22-sample slabs of the same U(-1,1) ComplexFloat32 IQ, 128 real taps; value = the reference's "
                      "production form (FFT overlap-save, firfilter.lua:320-398; self-contained Float32 Stockham FFT, not FFTW) on the fastest "
                      "OpenMP thread count; forms.dot_product = one SIMD dot product per output (firfilter.lua:129-145); single_core = 1 thread "
                      "(the reference gives a block one core); 5 trials each, mean and sigma (luaradio_benchmark.lua:10-13)"}


def verify_fir_output(torch, x, y, n, taps, fir_mode):
    """Check the output of the LAST timed step against the oracle on slabs of 2^18 samples at spread offsets (first, middle, last,
    three more).  Every step filters the same vector with the history carried from the previous step, so the samples before
    x[0] are the tail of x.  fft mode: <= 1e-6 of the f64 oracle; direct mode: bit-exact against the fmaf-chain oracle."""
    import numpy as np
    from oracle import oracle as O
    M, ln = len(taps), 1 << 18
    offs = sorted({0, n // 2 - ln // 2, n - ln, (n // 7) & ~1, (3 * n // 5) | 1, (n // 2) - 64})
    worst, exact = 0.0, True
    for o in offs:
        o = max(0, min(o, n - ln))
        if o >= M - 1:
            xs = x[2 * (o - (M - 1)):2 * (o + ln)].cpu().numpy().view(np.complex64)
        else:
            xs = torch.cat([x[2 * (n - (M - 1) + o):], x[:2 * (o + ln)]]).cpu().numpy().view(np.complex64)
        got = y[2 * o:2 * (o + ln)].cpu().numpy().view(np.complex64)
        ref = O.FIR(taps, True, mode=O.MODE_F64).process(xs)[M - 1:]
        worst = max(worst, float(np.max(np.abs(got - ref))))
        if fir_mode == "direct":
            exact = exact and bool(np.array_equal(got, O.FIR(taps, True, mode=O.MODE_FMA).process(xs)[M - 1:]))
    ok = worst <= 1e-6 and (exact or fir_mode != "direct")
    return {"verified": bool(ok), "max_err": worst, "bit_exact_vs_fmaf_oracle": exact if fir_mode == "direct" else None,
            "verify": "output of the last timed step vs oracle (f64 mode%s) on %d slabs of 2^18 samples at offsets %s" %
                      (", and bit-compared with the fmaf-chain mode" if fir_mode == "direct" else "", len(offs), offs)}


def wbfm_chain_report(lr, L, torch, dev, with_cpu):
    """second half of BASELINE.json's metric (configs[2]) inside the default bench line: the WBFM-mono receiver chain,
    device-resident, 2^26 synthetic FM IQ samples per step, HIP-event timed; with_cpu also runs the oracle chain (1 core)
    on the first 2^20 samples for the RMS error and the CPU rate."""
    import numpy as np
    fs, n = 1102500.0, 1 << 26
    t = torch.arange(n, dtype=torch.float64, device=dev) / fs
    m = 0.5 * torch.sin(2 * np.pi * 1e3 * t) + 0.5 * torch.sin(2 * np.pi * 5e3 * t)
    ph = 2 * np.pi * 250e3 * t + 2 * np.pi * 75e3 / fs * torch.cumsum(m, 0)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.stack([torch.cos(ph).float(), torch.sin(ph).float()], 1).reshape(-1)
    x += 0.01 * (torch.rand(2 * n, dtype=torch.float32, device=dev, generator=g) * 2 - 1)
    del t, m, ph
    rx = lr.wbfm_mono_receiver(fs, -250e3)
    cap = rx.max_output(n)
    y = torch.empty(cap + 16, dtype=torch.float32, device=dev)
    steps = 20
    t_ramp = time.perf_counter()                  # clock ramp + warm-up, untimed (see main())
    while time.perf_counter() - t_ramp < 0.15:
        for _ in range(4):
            rx.process_device(x.data_ptr(), n, y.data_ptr(), cap)
        torch.cuda.synchronize()
    rx.reset()                                    # the timed steps then start at absolute sample 0: the last one can be checked against the oracle
    tm = L.lrhip_timer_create()
    L.lrhip_timer_start(tm)
    got_n = 0
    for _ in range(steps):
        got_n = rx.process_device(x.data_ptr(), n, y.data_ptr(), cap)
    L.lrhip_timer_stop(tm)
    torch.cuda.synchronize()
    ms = L.lrhip_timer_elapsed_ms(tm) / steps
    L.lrhip_timer_destroy(tm)
    rep = {"workload": "configs[2]: Tuner(-250e3, 200e3, 5) -> FrequencyDiscriminator(1.25) -> Lowpass(128, 15e3) -> FMDeemphasis(75e-6) -> "
                       "Downsampler(5), 2^26 RF samples per step, device-resident",
           "value": round(n / ms / 1e3, 1), "unit": "MSamples/s (RF samples in)", "ms_per_step": round(ms, 4), "launches": rx.chain.last_launches,
           "kernel": "rx_fused_kernel (kernels_rx.h): tuner tiles -> discriminator -> batch window in LDS -> audio filter + recurrence, one launch",
           "algorithmic_GB/s": round(8.16 * n / ms / 1e6, 1)}
    rep["roofline_frac"] = round(8.16 * n / ms / 1e6 / HBM_PEAK_GBS, 4)
    if with_cpu:
        rep.update(verify_wbfm_chain(torch, x, y, got_n, n, (steps - 1) * n, fs, -250e3))
    # the same receiver on U(-1, 1) noise (one harness had timed this input 10 % slower): same clock state, same loop, both inputs in the line.
    # profiles/r04_rx_input_dependence.txt: identical instruction and cycle counts for the two inputs - the difference was the clock ramp of the other harness
    g2 = torch.Generator(device=dev).manual_seed(8)
    xn = torch.rand(2 * n, dtype=torch.float32, device=dev, generator=g2) * 2 - 1
    rxn = lr.wbfm_mono_receiver(fs, -250e3)
    t_ramp = time.perf_counter()                  # the oracle check above left the GPU idle for seconds: the same untimed clock ramp as the FM leg
    while time.perf_counter() - t_ramp < 0.15:
        for _ in range(4):
            rxn.process_device(xn.data_ptr(), n, y.data_ptr(), cap)
        torch.cuda.synchronize()
    tm = L.lrhip_timer_create()
    L.lrhip_timer_start(tm)
    for _ in range(steps):
        rxn.process_device(xn.data_ptr(), n, y.data_ptr(), cap)
    L.lrhip_timer_stop(tm)
    torch.cuda.synchronize()
    ms_n = L.lrhip_timer_elapsed_ms(tm) / steps
    L.lrhip_timer_destroy(tm)
    rep["on_uniform_noise_input"] = {"ms_per_step": round(ms_n, 4), "value": round(n / ms_n / 1e3, 1), "unit": "MSamples/s (RF samples in)",
                                     "roofline_frac": round(8.16 * n / ms_n / 1e6 / HBM_PEAK_GBS, 4), "ratio_to_fm_signal": round(ms_n / ms, 3)}
    del xn
    rep["from_u8_records"] = wbfm_u8_report(lr, L, torch, dev, x, n, fs, steps)
    return rep


def wbfm_u8_report(lr, L, torch, dev, x, n, fs, steps):
    """configs[2] says "fed from IQ file source": the same receiver behind IQFileSource's format stage for unsigned 8-bit records (RTL-SDR captures), the
    records resident in HBM.  The single launch reads the 2-byte records itself (kernels_rx.h, U8).  Checked bit for bit against the ComplexFloat32
    receiver (itself held to the oracle chain above) fed the same records converted by the stand-alone file-format kernel."""
    import numpy as np
    from luaradio_amd import _lib
    raw = torch.clamp(torch.round(x * 0.5 * 127.5 + 127.5), 0, 255).to(torch.uint8)      # the test signal at half scale as u8 (I, Q) records
    src = lr.IQFileSource(bytes(16), "u8", fs)
    src.initialize()
    blocks = [src, lr.FrequencyTranslatorBlock(-250e3), lr.LowpassFilterBlock(128, 100e3), lr.DownsamplerBlock(5), lr.FrequencyDiscriminatorBlock(1.25),
              lr.LowpassFilterBlock(128, 15e3), lr.FMDeemphasisFilterBlock(75e-6), lr.DownsamplerBlock(5)]
    r, t = src.get_rate(), src.get_output_type()
    for b in blocks[1:]:
        b.rate = r
        b.differentiate([t])
        b.initialize()
        r, t = b.get_rate(), b.get_output_type()
    chain = lr.Chain(blocks)
    cap = chain.max_output(n)
    y8 = torch.empty(cap + 16, dtype=torch.float32, device=dev)
    for _ in range(3):
        chain.process_device(raw.data_ptr(), n, y8.data_ptr(), cap)
    torch.cuda.synchronize()
    chain.reset()
    tm = L.lrhip_timer_create()
    L.lrhip_timer_start(tm)
    got = 0
    for _ in range(steps):
        got = chain.process_device(raw.data_ptr(), n, y8.data_ptr(), cap)
    L.lrhip_timer_stop(tm)
    torch.cuda.synchronize()
    ms = L.lrhip_timer_elapsed_ms(tm) / steps
    L.lrhip_timer_destroy(tm)
    launches = chain.last_launches
    # the ComplexFloat32 receiver on the converted records, the same number of steps (state carried alike), compared on the whole last output
    q = L.lrhip_format_convert_create(b"u8", 1)
    xc = torch.empty(2 * n, dtype=torch.float32, device=dev)
    _lib.check(L.lrhip_stage_execute_device(q, raw.data_ptr(), n, xc.data_ptr(), n), "format")
    L.lrhip_stage_destroy(q)
    ref = lr.wbfm_mono_receiver(fs, -250e3)
    yc = torch.empty(cap + 16, dtype=torch.float32, device=dev)
    gc = 0
    for _ in range(steps):
        gc = ref.process_device(xc.data_ptr(), n, yc.data_ptr(), cap)
    torch.cuda.synchronize()
    same = bool(got == gc and torch.equal(y8[:got].view(torch.int32), yc[:gc].view(torch.int32)))
    return {"ms_per_step": round(ms, 4), "value": round(n / ms / 1e3, 1), "unit": "MSamples/s (RF records in)", "launches": launches,
            "algorithmic_bytes_per_sample": 2.16, "algorithmic_GB/s": round(2.16 * n / ms / 1e6, 1),
            "verified": same, "verify": "audio of the last of %d steps bit-equal to the ComplexFloat32 receiver fed the records converted by the file-format "
                                        "kernel (%d audio samples)" % (steps, got)}


def verify_wbfm_chain(torch, x, y, got_n, n, base, fs, offset, nslabs=8, slab_rf=262150, warm_rf=100000):
    """The audio the LAST TIMED STEP wrote (y, got_n samples) for the whole 2^26-sample vector against the oracle chain (composition of the
    pinned per-block restatements) on `nslabs` slabs spread from the first to the last sample.  Every step runs the same vector with the
    state carried from the step before, so the last step covers absolute samples base .. base + n and the samples in front of x[0] are the
    tail of x.  A slab runs the oracle from zero state about `warm_rf` RF samples early - at an absolute sample that is a multiple of 25,
    both decimations (the de-emphasis pole 0.941^4000 and the FIR transients are long gone; the discriminator does not see the constant
    phase the oracle's rotator is off by) - and compares the following slab_rf / 25 audio samples.  Also times the oracle (1 core)."""
    import numpy as np
    from oracle import oracle as O
    first_audio = (base + 24) // 25                          # absolute index of the step's first audio sample
    starts = [0] + [int((n - slab_rf) * k / (nslabs - 1)) for k in range(1, nslabs)]
    se, cnt, worst, cpu_s, cpu_n = 0.0, 0, 0.0, 0.0, 0
    for s0 in starts:
        lo = s0 - warm_rf
        if base + lo < 0:
            lo = -base                                       # the stream starts here: zero state is the true state
        lo -= (base + lo) % 25                               # oracle output i is absolute audio sample (base + lo) / 25 + i
        hi = min(n, s0 + slab_rf)
        if lo < 0:
            xs = torch.cat([x[2 * (n + lo):], x[:2 * hi]]).cpu().numpy().view(np.complex64)
        else:
            xs = x[2 * lo:2 * hi].cpu().numpy().view(np.complex64)
        ch = O.wbfm_mono_chain(fs, offset, mode=O.MODE_LUA, rot_mode=O.MODE_F64)
        t0 = time.perf_counter()
        want = ch.process(xs)
        cpu_s += time.perf_counter() - t0
        cpu_n += len(xs)
        skip = (base + s0 + 24) // 25 - (base + lo) // 25    # oracle samples in front of the slab
        want = want[skip:]
        a0 = (base + s0 + 24) // 25 - first_audio
        got = y[a0:min(got_n, a0 + len(want))].cpu().numpy()
        m = min(len(got), len(want))
        err = got[:m].astype(np.float64) - want[:m].astype(np.float64)
        se += float(np.sum(err ** 2))
        cnt += m
        worst = max(worst, float(np.max(np.abs(err))))
    rms = (se / max(cnt, 1)) ** 0.5
    return {"rms_err_vs_oracle": rms, "max_err_vs_oracle": worst, "verified": bool(rms <= 1e-5 and got_n > 0 and cnt > 60000),
            "verify": "audio written by the LAST timed step (state carried through all %d steps) vs the oracle chain on %d slabs of %d RF samples from the "
                      "first to the last sample (%d audio samples compared), bar: RMS <= 1e-5" % (base // n + 1, len(starts), slab_rf, cnt),
            "cpu_baseline": {"value": round(cpu_n / cpu_s / 1e6, 2), "unit": "MSamples/s", "cores": 1, "kind": "port",
                             "sample": "oracle chain (per-block restatement of the reference's Lua arithmetic) on the %d verification slabs, %d RF samples" % (len(starts), cpu_n)}}


def clock_ramp(torch, step, seconds=0.15):
    """Untimed launches in front of a leg's timed steps, as the headline has them (prewarm_ms): the leg in front ends with seconds of host-side verification,
    and the first launches of an idle GPU run at reduced clocks (channelizer: 1.27-1.30 ms cold against a traced 1.11-1.21 ms for the same kernel)."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            step()
        torch.cuda.synchronize()


def channelizer_report(lr, L, torch, dev, with_cpu):
    """BASELINE.json configs[4]: 64-channel critically sampled filterbank, 1024-tap prototype, as one dense GEMM on the f32 matrix
    cores, 2^24 ComplexFloat32 samples per step.  Reports TFLOP/s against the 157.3 TFLOP/s f32 MFMA peak (the matrix-pipe busy
    fraction from counters is in profiles/), and the error against K oracle chains Translator -> FIR -> Downsampler."""
    import numpy as np
    from luaradio_amd import types
    n, K, M = 1 << 24, 64, 1024
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand(2 * n, dtype=torch.float32, device=dev, generator=g) * 2 - 1
    ch = lr.PolyphaseChannelizerBlock(K)
    ch.rate = 1102500.0
    ch.differentiate([types.ComplexFloat32])
    ch.initialize()
    cap = ch.max_output(n)
    y = torch.empty(2 * cap + 64, dtype=torch.float32, device=dev)
    ch.process_device(x.data_ptr(), n, y.data_ptr(), cap)
    clock_ramp(torch, lambda: ch.process_device(x.data_ptr(), n, y.data_ptr(), cap))
    steps = 10
    tm = L.lrhip_timer_create()
    L.lrhip_timer_start(tm)
    for _ in range(steps):
        ch.process_device(x.data_ptr(), n, y.data_ptr(), cap)
    L.lrhip_timer_stop(tm)
    torch.cuda.synchronize()
    ms = L.lrhip_timer_elapsed_ms(tm) / steps
    L.lrhip_timer_destroy(tm)
    tf = 8.0 * M * n / ms / 1e9
    rep = {"workload": "configs[4]: %d-channel polyphase filterbank, %d-tap prototype, dense batched GEMM [T x 2M].[2M x 2K] on v_mfma_f32_16x16x4_f32, "
                       "2^24 ComplexFloat32 samples per step" % (K, M),
           "value": round(n / ms / 1e3, 1), "unit": "MSamples/s (input)", "ms_per_step": round(ms, 4), "dtype": "f32",
           "roofline": {"bound": "mfma", "achieved": round(tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / FP32_PEAK_TFLOPS, 4),
                        "flops_per_sample": 8 * M, "mfma_busy_counter": "profiles/ (SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CU_CYCLES)"}}
    if with_cpu:
        from oracle import oracle as O
        # the output of the LAST timed step (every step starts from the state the previous one left: the 1023 samples in front of x[0] are the
        # tail of x), 96 frames each at the start, in the middle and at the end of the 2^24-sample vector, channels 0, 7, .., 63
        taps = ch.taps
        frames, pre = 96, ((M - 1 + K - 1) // K) * K
        se, cnt, worst = 0.0, 0, 0.0
        nfr = n // K
        for f0 in (0, nfr // 2 - frames // 2, nfr - frames):
            lo = f0 * K - pre
            if lo < 0:
                xs = torch.cat([x[2 * (n + lo):], x[:2 * (f0 + frames) * K]]).cpu().numpy().view(np.complex64)
            else:
                xs = x[2 * lo:2 * (f0 + frames) * K].cpu().numpy().view(np.complex64)
            got = y[2 * f0 * K:2 * (f0 + frames) * K].cpu().numpy().view(np.complex64).reshape(frames, K)
            for c in range(0, K, 7):
                # the oracle's rotator starts at phase 0 on sample lo; the block's at the absolute sample index: e^{-j 2 pi c lo / K} = 1 (lo is a multiple of K)
                want = O.Chain([O.Rotator(-2 * np.pi * c / K, O.MODE_F64), O.FIR(taps, True, O.MODE_F64), O.Downsampler(K, True)]).process(xs)[pre // K:]
                e = np.abs(got[:, c].astype(np.complex128) - want[:frames].astype(np.complex128))
                se += float(np.sum(e ** 2)); cnt += len(e); worst = max(worst, float(e.max()))
        rep.update({"rms_err_vs_oracle_chains": (se / cnt) ** 0.5, "max_err_vs_oracle_chains": worst, "verified": bool(worst < 2e-6),
                    "verify": "output of the last timed step: %d frames each at the start, the middle and the end of the 2^24-sample vector, channels 0,7,..,63 vs oracle "
                              "chains FrequencyTranslator(-c/K) -> FIRFilter(h) -> Downsampler(K) in f64 (no reference block exists: parity unpinned, SURVEY.md 8c-ii)" % frames})
    return rep


def verify_tuner_branch(torch, tun, run, x, n, fs, offset, bandwidth, decim, slab=1 << 17, warm=2000):
    """One fan-out branch against the oracle Tuner (radio/composites/tuner.lua:32-48 restated): the branch is reset, run() pushes the slab once
    more, and its ComplexFloat32 output is compared on three slabs (first / middle / last samples).  The oracle's rotator starts at phase 0 on
    the first sample it is given, the block's at the absolute sample index: the oracle's output is turned by exp(j omega lo) - the filter is linear."""
    import numpy as np
    from oracle import oracle as O
    tun.reset()
    out = run()
    torch.cuda.synchronize()
    worst, cnt = 0.0, 0
    for s0 in (0, (n // 2) // decim * decim, (n - slab) // decim * decim):
        lo = max(0, s0 - warm) // decim * decim
        xs = x[2 * lo:2 * (s0 + slab)].cpu().numpy().view(np.complex64)
        want = O.tuner(offset, bandwidth, decim, fs, mode=O.MODE_F64, rot_mode=O.MODE_F64).process(xs)[(s0 - lo) // decim:]
        turn = (offset / fs * lo) % 1.0
        want = want.astype(np.complex128) * np.exp(2j * np.pi * turn)
        got = out[2 * (s0 // decim):2 * (s0 // decim + len(want))].cpu().numpy().view(np.complex64)
        m = min(len(got), len(want))
        worst = max(worst, float(np.max(np.abs(got[:m].astype(np.complex128) - want[:m]))))
        cnt += m
    return {"verified": bool(worst <= 2e-6 and cnt > 3 * slab // decim - 16), "max_err_vs_oracle": worst,
            "verify": "branch output (after a reset, one more push of the slab) vs the oracle Tuner in f64 on 3 slabs of 2^17 RF samples (first / middle / last), %d outputs, bar 2e-6" % cnt}


def fm_recording(torch, dev, a, b, fs=1102500.0, block=1 << 22):
    """samples [a, b) of ONE long synthetic FM recording (SURVEY.md 8d C3 recipe), the same values whichever rank / partition asks: the phase is the
    closed-form integral of the two-tone message, the noise comes from one generator per block of 2^22 samples (seed = block index)"""
    import numpy as np
    i = torch.arange(a, b, dtype=torch.float64, device=dev)
    t = i / fs
    integ = -0.5 * torch.cos(2 * np.pi * 1e3 * t) / (2 * np.pi * 1e3) - 0.5 * torch.cos(2 * np.pi * 5e3 * t) / (2 * np.pi * 5e3)
    ph = 2 * np.pi * ((250e3 * t) % 1.0) + 2 * np.pi * 75e3 * integ
    x = torch.stack([torch.cos(ph).float(), torch.sin(ph).float()], 1).reshape(-1)
    del i, t, integ, ph
    for blk in range(a // block, (b + block - 1) // block):
        g = torch.Generator(device=dev).manual_seed(100000 + blk)
        nz = torch.rand(2 * block, dtype=torch.float32, device=dev, generator=g) * 2 - 1
        lo, hi = max(a, blk * block), min(b, (blk + 1) * block)
        x[2 * (lo - a):2 * (hi - a)] += 0.01 * nz[2 * (lo - blk * block):2 * (hi - blk * block)]
    return x


def verify_partition(torch, dev, y, got_n, a, b, fs, offset, slab_rf=131075, warm_rf=100000):
    """time partition [a, b) of the recording: its first and its last audio samples against the oracle chain run on the SAME recording from zero
    state `warm_rf` samples early (so the oracle crosses the partition boundary, which the partition itself only saw through its replayed halo)"""
    import numpy as np
    from oracle import oracle as O
    worst, se, cnt = 0.0, 0.0, 0
    first_audio = (a + 24) // 25
    for s0 in (a, max(a, b - slab_rf)):
        lo = max(0, s0 - warm_rf)
        lo -= lo % 25
        hi = min(b, s0 + slab_rf)
        xs = fm_recording(torch, dev, lo, hi, fs).cpu().numpy().view(np.complex64)
        want = O.wbfm_mono_chain(fs, offset, mode=O.MODE_LUA, rot_mode=O.MODE_F64).process(xs)[(s0 + 24) // 25 - lo // 25:]
        a0 = (s0 + 24) // 25 - first_audio
        got = y[a0:min(got_n, a0 + len(want))].cpu().numpy()
        m = min(len(got), len(want))
        err = got[:m].astype(np.float64) - want[:m].astype(np.float64)
        se += float(np.sum(err ** 2)); cnt += m
        worst = max(worst, float(np.max(np.abs(err))))
    rms = (se / max(cnt, 1)) ** 0.5
    return bool(rms <= 1e-5 and cnt > 2 * (slab_rf // 25) - 64), rms, worst


def fanout_report(lr, L, torch, dev):
    """BASELINE.json configs[3] degenerate at N = 1: the per-GPU branch of the fan-out (one Tuner(offset_0, 100e3, 5) on the slab the
    source GPU would broadcast), 2^26 samples per step; the broadcast itself only exists for N > 1 (bench.py --workload fanout)."""
    from luaradio_amd import fanout, types
    n, fs = 1 << 26, 1102500.0
    g = torch.Generator(device=dev).manual_seed(4)
    x = torch.rand(2 * n, dtype=torch.float32, device=dev, generator=g) * 2 - 1
    tun = lr.TunerBlock(fanout.branch_offsets(8)[0], 100e3, 5)
    tun.rate = fs
    tun.differentiate([types.ComplexFloat32])
    tun.initialize()
    fo = fanout.FanOut(None, 0, 1, 1, {0: fanout.DeviceBranch(tun, n)}, src=0)
    fo.push(x)
    clock_ramp(torch, lambda: fo.push(x))
    steps = 10
    tm = L.lrhip_timer_create()
    L.lrhip_timer_start(tm)
    for _ in range(steps):
        fo.push(x)
    L.lrhip_timer_stop(tm)
    torch.cuda.synchronize()
    ms = L.lrhip_timer_elapsed_ms(tm) / steps
    L.lrhip_timer_destroy(tm)
    ver = verify_tuner_branch(torch, tun, lambda: fo.push(x)[0], x, n, fs, fanout.branch_offsets(8)[0], 100e3, 5)
    rec = fanout_records_report(lr, L, torch, dev, x, n, fs, fanout.branch_offsets(8)[0])
    return {"from_u8_records": rec,
            "workload": "configs[3] at N = 1: one fan-out branch Tuner(-350e3, 100e3, 5) on a 2^26-sample slab (no broadcast with one GPU)",
            "value": round(n / ms / 1e3, 1), "unit": "MSamples/s (branch input)", "ms_per_step": round(ms, 4), **ver,
            "algorithmic_GB/s": round(9.6 * n / ms / 1e6, 1), "roofline_frac": round(9.6 * n / ms / 1e6 / HBM_PEAK_GBS, 4),
            "xgmi_link_bound_MSps": 19125.0,
            "note": "for N > 1 every receiving GPU is bounded by one xGMI link: 153 GB/s / 8 B = 19.1 GS/s of ComplexFloat32, far below this branch rate"}


def fanout_records_report(lr, L, torch, dev, x, n, fs, offset):
    """the same branch when the source is an IQ file: the slab that would be broadcast holds the raw u8 records (2 B per sample on every xGMI link
    instead of 8) and the branch chain starts with IQFileSource's format stage, which lrhip_chain_create folds into the Tuner's launch.  Checked bit for bit
    against the ComplexFloat32 Tuner (held to the oracle above) on the records converted by the file-format kernel."""
    from luaradio_amd import _lib, fanout, types
    raw = torch.clamp(torch.round(x * 127.5 + 127.5), 0, 255).to(torch.uint8)

    def tuner(head):
        blocks = head + [lr.FrequencyTranslatorBlock(offset), lr.LowpassFilterBlock(128, 100e3), lr.DownsamplerBlock(5)]
        r, t = fs, types.ComplexFloat32
        for b in blocks[len(head):]:
            b.rate = r
            b.differentiate([t])
            b.initialize()
            r, t = b.get_rate(), b.get_output_type()
        return lr.Chain(blocks)

    src = lr.IQFileSource(bytes(16), "u8", fs)
    src.initialize()
    chain = tuner([src])
    br = fanout.DeviceBranch(chain, n)
    fo = fanout.FanOut(None, 0, 1, 1, {0: br}, src=0)
    clock_ramp(torch, lambda: fo.push(raw))
    chain.reset()                                  # (the ramp's launch count depends on the clock: the verified state below is one warm-up push + the timed steps)
    fo.push(raw)
    steps = 10
    tm = L.lrhip_timer_create()
    L.lrhip_timer_start(tm)
    for _ in range(steps):
        got = fo.push(raw)[0]
    L.lrhip_timer_stop(tm)
    torch.cuda.synchronize()
    ms = L.lrhip_timer_elapsed_ms(tm) / steps
    L.lrhip_timer_destroy(tm)
    launches = chain.last_launches
    q = L.lrhip_format_convert_create(b"u8", 1)
    xc = torch.empty(2 * n, dtype=torch.float32, device=dev)
    _lib.check(L.lrhip_stage_execute_device(q, raw.data_ptr(), n, xc.data_ptr(), n), "format")
    L.lrhip_stage_destroy(q)
    ref = fanout.DeviceBranch(tuner([]), n)
    want = None
    for _ in range(steps + 1):                     # the same number of pushes: the rotator phase and the filter history advance alike
        want = ref.process(xc)
    torch.cuda.synchronize()
    same = bool(got.numel() == want.numel() and torch.equal(got.view(torch.int32), want.view(torch.int32)))
    return {"ms_per_step": round(ms, 4), "value": round(n / ms / 1e3, 1), "unit": "MSamples/s (branch input records)", "launches": launches,
            "xgmi_link_bound_MSps": 76500.0, "verified": same,
            "verify": "branch output of the last push bit-equal to the ComplexFloat32 Tuner on the converted records (%d outputs)" % (got.numel() // 2),
            "note": "2 B per sample on the link: 153 GB/s / 2 B = 76.5 GS/s per receiving GPU instead of 19.1"}


def host_path_report(lr, L, torch, dev):
    """VERDICT r03 missing 5 / 6: what a LuaRadio flow graph sees, PCIe included - never `value`.  (a) configs[2] "fed from IQ file source": a file in
    the page cache is read in IQFileSource's 8 192-sample chunks (radio/blocks/sources/iqfile.lua:52) and in the pipe's 131 072-sample chunks
    (radio/core/pipe.lua:495-533) and pushed into the receiver chain's pinned ring (lrhip_chain_push, batches of 2^20 samples, depth 3) - u8 records
    (2 B per sample on the link) and ComplexFloat32 (8 B); (b) a STAND-ALONE block, LowpassFilterBlock(128) cf32 -> cf32 through lrhip_stage_execute
    with 2^20-sample vectors: both directions cross the link; with the caller's page-aligned vectors registered (lrhip_host_register: DMA from / to
    them, no staging copy) and without.  Every leg's output is compared bit for bit with the device-resident run of the same batches."""
    import ctypes as C
    import tempfile
    import numpy as np
    from luaradio_amd import _lib, types
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from iqfile_wbfm_mono import build_chain
    LINK = 64.0                                        # PCIe 5.0 x16, GB/s per direction (nominal)
    n, fs, batch = 1 << 24, 1102500.0, 1 << 20
    rng = np.random.default_rng(11)
    rep = {"link_GB/s_nominal": LINK, "samples": n, "batch_samples": batch, "ring_depth": 3}
    tmp = tempfile.mkdtemp(prefix="lrhip_bench_")
    try:
        # ---- (a) file -> receiver
        raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        cf = (((raw.astype(np.float32) - 127.5) / 127.5)).view(np.complex64)
        files = {"u8": (os.path.join(tmp, "iq.u8"), raw, 2), "f32le": (os.path.join(tmp, "iq.f32"), cf.view(np.uint8), 8)}
        for fmt, (path, data, rec) in files.items():
            with open(path, "wb") as f:
                f.write(data.tobytes())
        legs = []
        for fmt, (path, data, rec) in files.items():
            # device-resident reference of the same batches (state carried alike): the bits the host path has to deliver
            _s, ref, _r = build_chain(bytes(16), fmt, fs, -250e3)
            dx = torch.from_numpy(data).to(dev)
            cap = ref.max_output(batch) + 64
            dy = torch.empty(cap, dtype=torch.float32, device=dev)
            want = []
            for a in range(0, n, batch):
                got = ref.process_device(dx.data_ptr() + a * rec, batch, dy.data_ptr(), cap)
                want.append(dy[:got].cpu().numpy().copy())
            want = np.concatenate(want)
            del dx
            for chunk in (8192, 131072):
                _s, ch, _r = build_chain(bytes(16), fmt, fs, -250e3)
                ch.set_ring(3, batch)
                buf = np.empty(chunk * rec, np.uint8)
                outs = []
                with open(path, "rb", buffering=0) as f:
                    f.readinto(buf)                    # page cache warm, first-touch of buf done
                    f.seek(0)
                    t0 = time.perf_counter()
                    while True:
                        got = f.readinto(buf)
                        if not got:
                            break
                        outs.append(ch.push(buf[:got]))
                    outs.append(ch.flush())
                    dt = time.perf_counter() - t0
                y = np.concatenate(outs)
                legs.append({"source": "%s IQ file (page cache) -> WBFM receiver" % fmt, "chunk_samples": chunk, "MSamples/s": round(n / dt / 1e6, 1),
                             "h2d_GB/s": round(rec * n / dt / 1e9, 2), "frac_of_link": round(rec * n / dt / 1e9 / LINK, 3),
                             "verified": bool(len(y) == len(want) and np.array_equal(y, want))})
            # the path of an IQFileSource absorbed into the chain (lua/radio/blocks/sources/file_hip.lua submit_raw): the library reads the records itself
            for _pass in range(2):                 # pass 0: warm-up (the ring's pinned slots, the copy threads), as the C driver does
                _s, ch, _r = build_chain(bytes(16), fmt, fs, -250e3)
                ch.set_ring(3, batch)
                outs, off = [], 0
                with open(path, "rb", buffering=0) as f:
                    t0 = time.perf_counter()
                    while True:
                        if ch.in_flight == 3:
                            outs.append(ch.collect())
                        got = ch.submit_fd(f.fileno(), off, batch)
                        if got == 0:
                            break
                        off += got * rec
                    while ch.in_flight:
                        outs.append(ch.collect())
                    dt = time.perf_counter() - t0
            y = np.concatenate(outs)
            legs.append({"source": "%s IQ file (page cache) -> WBFM receiver, lrhip_chain_submit_fd (the library reads the file)" % fmt, "chunk_samples": batch,
                         "MSamples/s": round(n / dt / 1e6, 1), "h2d_GB/s": round(rec * n / dt / 1e9, 2), "frac_of_link": round(rec * n / dt / 1e9 / LINK, 3),
                         "verified": bool(len(y) == len(want) and np.array_equal(y, want))})
        rep["file_to_receiver"] = legs
        # ---- (b) stand-alone block, both directions
        def aligned(count, dtype):
            raw_b = np.empty(count * np.dtype(dtype).itemsize + 4096, np.uint8)
            off = (-raw_b.ctypes.data) % 4096
            return raw_b[off:off + count * np.dtype(dtype).itemsize].view(dtype)
        vec = 1 << 20
        x = aligned(n, np.complex64)
        x[:] = cf
        y = aligned(n, np.complex64)
        blocks = {}
        for name in ("staged", "registered"):
            blk = lr.LowpassFilterBlock(128, 15e3)
            blk.use_fft = 2
            blk.rate = 220500.0
            blk.differentiate([types.ComplexFloat32])
            blk.initialize()
            blocks[name] = blk
        def run(blk):
            q = blk.stage_handle()
            t0 = time.perf_counter()
            for a in range(0, n, vec):
                got = L.lrhip_stage_execute(q, x[a:a + vec].ctypes.data_as(C.c_void_p), vec, y[a:a + vec].ctypes.data_as(C.c_void_p), vec)
                assert got == vec
            return time.perf_counter() - t0
        dxx = torch.from_numpy(x.view(np.float32).copy()).to(dev)
        dyy = torch.empty(2 * n, dtype=torch.float32, device=dev)
        refb = lr.LowpassFilterBlock(128, 15e3)
        refb.use_fft = 2
        refb.rate = 220500.0
        refb.differentiate([types.ComplexFloat32])
        refb.initialize()
        # the host path cuts a 2^20-sample call into pipelined pieces of at least 2^19 samples (chain.h HOST_PIECE_MIN) on the filter's own block grid
        # (FirStage::align: multiples of 1024 - 128 = 896 samples for 128 taps); a piece is a chunk like any other - its first block takes the sample in
        # front of its 127-sample history as zero - so the device-resident reference takes the same cuts and has to agree bit for bit
        pieces = min(8, vec >> 19) if vec >= (1 << 20) else 1
        per = -(-(vec // pieces) // 896) * 896
        for a in range(0, n, vec):
            o = 0
            while o < vec:
                m = min(per, vec - o)
                refb.process_device(dxx.data_ptr() + 8 * (a + o), m, dyy.data_ptr() + 8 * (a + o), m)
                o += m
        want = dyy.cpu().numpy().view(np.complex64)
        # round 5: with BOTH vectors registered the call is not cut at all - the kernels read and write the caller's vectors in place (host_execute's direct mode,
        # chain.h) - so that leg's reference is the device-resident run of the whole 2^20-sample vectors
        refw = lr.LowpassFilterBlock(128, 15e3)
        refw.use_fft = 2
        refw.rate = 220500.0
        refw.differentiate([types.ComplexFloat32])
        refw.initialize()
        for a in range(0, n, vec):
            refw.process_device(dxx.data_ptr() + 8 * a, vec, dyy.data_ptr() + 8 * a, vec)
        want_whole = dyy.cpu().numpy().view(np.complex64)
        res = {}
        for name, blk in blocks.items():
            if name == "registered":
                _lib.check(L.lrhip_host_register(x.ctypes.data_as(C.c_void_p), x.nbytes), "register")
                _lib.check(L.lrhip_host_register(y.ctypes.data_as(C.c_void_p), y.nbytes), "register")
            run(blk)
            blk.reset()
            dt = run(blk)
            res[name] = {"MSamples/s": round(n / dt / 1e6, 1), "each_direction_GB/s": round(8.0 * n / dt / 1e9, 2), "frac_of_link": round(8.0 * n / dt / 1e9 / LINK, 3),
                         "verified": bool(np.array_equal(y, want) or (name == "registered" and np.array_equal(y, want_whole)))}
            if name == "registered":
                res[name]["in_place"] = bool(np.array_equal(y, want_whole) and not np.array_equal(y, want))
                L.lrhip_host_unregister(x.ctypes.data_as(C.c_void_p))
                L.lrhip_host_unregister(y.ctypes.data_as(C.c_void_p))
        rep["standalone_lowpass_cf32"] = dict(res, vector_samples=vec, note="LowpassFilterBlock(128, 15e3), overlap-save arithmetic, lrhip_stage_execute: host vector "
                                              "in, host vector out; staged: a call travels as up to 8 pipelined pieces (H2D, kernels, D2H on three streams); registered: the kernels read and write the "
                                              "caller's vectors across the link themselves (direct mode, one launch per call)")
        # ---- (c) the same paths THROUGH C (tools/host_path_driver.cpp, built by __graft_entry__.build()): no interpreter in the loop, so the per-call cost of
        # the library itself is visible next to the Python legs above (whose 8 192-sample figures are ~8.5 us of Python per push)
        drv = os.path.join(ROOT, "tools", "host_path_driver")
        if os.path.exists(drv):
            import subprocess
            try:
                p = subprocess.run([drv, str(n), tmp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
                lines = [json.loads(ln) for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
                for ln in lines:
                    if "h2d_GB/s" in ln:
                        ln["frac_of_link"] = round(ln["h2d_GB/s"] / LINK, 3)
                    if "each_direction_GB/s" in ln:
                        ln["frac_of_link"] = round(ln["each_direction_GB/s"] / LINK, 3)
                # the legs of one input format compute the same audio (to the chain's stated chunking dependence, <= 2e-7 per sample): their checksums agree
                agree = True
                for fmt in ("u8", "f32le"):
                    cs = [ln["checksum"] for ln in lines if ln.get("format") == fmt]
                    na = {ln["audio_samples"] for ln in lines if ln.get("format") == fmt}
                    agree = agree and len(na) == 1 and (max(cs) - min(cs)) <= 1e-3 * max(1.0, max(abs(c) for c in cs))
                rep["through_c"] = {"legs": lines, "rc": p.returncode, "checksums_agree": bool(agree and p.returncode == 0),
                                    "note": "tools/host_path_driver.cpp: push = read(2) + lrhip_chain_push per chunk; ring = read(2) into lrhip_chain_ring_input; "
                                            "fd = lrhip_chain_submit_fd (the library preads on its copy threads); best of two timed passes after a warm-up pass"}
                if p.returncode != 0:
                    rep["through_c"]["stderr"] = p.stderr.decode(errors="replace")[-400:]
            except Exception as e:          # noqa: BLE001 - a leg that cannot run is reported, not fatal
                rep["through_c"] = {"error": "%s: %s" % (type(e).__name__, e)}
        else:
            rep["through_c"] = {"error": "tools/host_path_driver not built (python __graft_entry__.py)"}
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
    rep["verified"] = all(l["verified"] for l in rep["file_to_receiver"]) and all(v["verified"] for k, v in rep["standalone_lowpass_cf32"].items() if isinstance(v, dict))
    return rep


def take_outputs(torch, arrays, budget):
    """--dump-outputs: device copies of {name: 2-D float32 tensor} as the last timed step left them (the spread trials run the step again).  An array
    larger than its share of `budget` is cut to a fixed sample of rows (numpy default_rng(0), sorted), whose positions go along as <name>_index."""
    import numpy as np
    share = budget // max(len(arrays), 1)
    out = {}
    for name, t in arrays.items():
        rows, row_bytes = t.shape[0], t.shape[1] * t.element_size()
        if rows * row_bytes <= share:
            out[name] = t.clone()
            continue
        idx = np.unique(np.random.default_rng(0).integers(0, rows, share // (row_bytes + 8)))
        out[name] = t[torch.from_numpy(idx).to(t.device)]
        out[name + "_index"] = idx.astype(np.float64)
    return out


def write_outputs(path, outs, prefix):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, v in outs.items():
        np.save(os.path.join(path, prefix + name + ".npy"), v.cpu().numpy() if hasattr(v, "cpu") else v)


def main():
    args = parse()
    self_launch(args)
    if args.launch_check:
        print(json.dumps({"launch_check": True, "rank": int(os.environ.get("RANK", "0")), "local_rank": int(os.environ.get("LOCAL_RANK", "0")),
                          "world": int(os.environ.get("WORLD_SIZE", "1")), "gpus": args.gpus}), flush=True)
        return
    import numpy as np
    import torch
    import luaradio_amd as lr
    from luaradio_amd import types

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    if args.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo")
    lr.init(local_rank)
    L = lr._lib.load()
    # launch on torch's current stream (its default stream has handle 0 = hipStreamLegacy for the library) so torch.cuda.synchronize()/barriers,
    # torch tensors handed to process_device() and the library's HIP events are all ordered on one stream
    lr.adopt_torch_stream()

    log2n = args.log2_samples or (28 if args.workload == "fir" else 26)
    n = 1 << log2n
    dev = torch.device("cuda", local_rank)
    gen = torch.Generator(device=dev).manual_seed(2 + rank)

    extra = {}
    if args.workload == "fir":
        # synthetic IQ: re/im ~ U(-1,1), generated on the device in 2^24-sample slabs
        x = torch.empty(2 * n, dtype=torch.float32, device=dev)
        slab = 1 << 25
        for o in range(0, 2 * n, slab):
            x[o:o + slab] = torch.rand(min(slab, 2 * n - o), dtype=torch.float32, device=dev, generator=gen) * 2 - 1
        y = torch.empty(2 * n, dtype=torch.float32, device=dev)
        fir_mode = "fft" if args.fir_mode == "auto" else args.fir_mode
        blk = lr.LowpassFilterBlock(128, 15e3)
        blk.use_fft = 2 if fir_mode == "fft" else 0
        blk.rate = 220500.0
        blk.differentiate([types.ComplexFloat32])
        blk.initialize()
        taps = blk.taps.copy()

        def step():
            got = blk.process_device(x.data_ptr(), n, y.data_ptr(), n)
            assert got == n

        def outputs():
            return {"fir_output": y.view(n, 2)}

        out_per_step = n
        alg_bytes = 16.0 * n
        flops = 4.0 * 128 * n if fir_mode == "direct" else 125.0 * n
        dominant = "fir_mfma_persistent_kernel<2,1,8,false,36>" if fir_mode == "direct" else "fir_fft_kernel<2,0>"
        config = {"workload": "configs[1]: 128-tap real-taps FIR (LowpassFilterBlock(128, 15e3) @ 220.5 kHz) on 2^%d synthetic "
                              "ComplexFloat32 IQ per GPU" % log2n,
                  "samples_per_step_per_gpu": n, "taps": 128, "kernel": dominant,
                  "algorithm": ("direct form, banded-Toeplitz product on the f32 matrix cores (bit-exact fmaf chain)" if fir_mode == "direct"
                                else "overlap-save, fused 1024-point FFT kernel (the reference's production form, firfilter.lua:320-398), <= 1e-6 of the f64 oracle"),
                  "parallelism": "independent streams x%d" % world}
    elif args.workload == "wbfm":
        fs = 1102500.0
        t = torch.arange(n, dtype=torch.float64, device=dev) / fs
        m = 0.5 * torch.sin(2 * np.pi * 1e3 * t) + 0.5 * torch.sin(2 * np.pi * 5e3 * t)
        ph = 2 * np.pi * 250e3 * t + 2 * np.pi * 75e3 / fs * torch.cumsum(m, 0)
        noise = torch.rand(2 * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1
        x = torch.stack([torch.cos(ph).float(), torch.sin(ph).float()], 1).reshape(-1) + 0.01 * noise
        del t, m, ph, noise
        rx = lr.wbfm_mono_receiver(fs, -250e3)
        cap = rx.max_output(n)
        y = torch.empty(cap + 16, dtype=torch.float32, device=dev)
        produced = []

        def step():
            produced.append(rx.process_device(x.data_ptr(), n, y.data_ptr(), cap))

        def outputs():
            return {"wbfm_audio": y[:produced[-1]].view(-1, 1)}

        out_per_step = n      # metric counts RF samples in; audio samples out reported in config
        alg_bytes = 8.16 * n
        flops = 167.0 * n
        config = {"workload": "configs[2]: examples/rtlsdr_wbfm_mono.lua chain (Tuner -> FrequencyDiscriminator -> Lowpass -> "
                              "FMDeemphasis -> Downsampler) on 2^%d synthetic FM IQ samples @ 1.1025 MS/s, device-resident" % log2n,
                  "samples_per_step_per_gpu": n, "counted": "RF input samples", "parallelism": "independent streams x%d" % world}
        dominant = "rx_fused_kernel (the whole receiver, one launch)"
    elif args.workload == "timeshard":
        # ONE recording of 2^log2n samples cut into `world` time partitions (second mode): rank r runs the receiver on its own
        # partition - lrhip_chain_start_at: seek to the aligned sample in front of (a - halo), replay, drop the replayed output - with no
        # exchange between the ranks.  Total work is fixed: "scaling": "strong".  One step = the whole job once.
        from luaradio_amd import timeshard
        fs = 1102500.0
        log2n = args.log2_samples or 28
        n_total = 1 << log2n
        rx = lr.wbfm_mono_receiver(fs, -250e3)
        align, halo = rx.shard_align(), rx.halo()
        pa, pb = timeshard.bounds(n_total, world, align)[rank]
        ps = timeshard.replay_start(pa, halo, align)
        x = fm_recording(torch, dev, ps, pb, fs)
        n = pb - ps
        cap = rx.max_output(n) + 16
        y = torch.empty(cap, dtype=torch.float32, device=dev)
        produced = []

        def step():
            assert rx.chain.start_at(pa) == ps
            produced.append(rx.process_device(x.data_ptr(), n, y.data_ptr(), cap))

        def outputs():
            return {"timeshard_audio": y[:produced[-1]].view(-1, 1)}

        out_per_step = n_total / world      # the job is the recording, whatever the number of ranks
        alg_bytes = 8.16 * (pb - pa)
        flops = 167.0 * (pb - pa)
        config = {"workload": "configs[2] chain on ONE synthetic FM recording of 2^%d samples cut into %d time partitions (lrhip_chain_start_at: halo %d samples "
                              "replayed per partition, boundaries on multiples of %d), one partition per GPU, no exchange" % (log2n, world, halo, align),
                  "samples_total": n_total, "counted": "RF input samples of the recording", "parallelism": "time partitions x%d" % world,
                  "partition_of_rank0": [pa, pb], "replayed_samples_rank0": pa - ps}
        dominant = "rx_fused_kernel"
    else:
        # fan-out: rank 0 owns the IQ slab; every step it is broadcast over RCCL/xGMI and each rank runs its own
        # Tuner branch (offsets -350 kHz .. +350 kHz step 100 kHz)
        fs = 1102500.0
        x = torch.empty(2 * n, dtype=torch.float32, device=dev)
        if rank == 0:
            x.copy_(torch.rand(2 * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1)
        from luaradio_amd import fanout
        nbranches = world
        offs = fanout.branch_offsets(8 if world <= 8 else world)
        mine = {}
        for b in fanout.local_branches(nbranches, world, rank):
            tun = lr.TunerBlock(offs[b % len(offs)], 100e3, 5)
            tun.rate = fs
            tun.differentiate([types.ComplexFloat32])
            tun.initialize()
            mine[b] = fanout.DeviceBranch(tun, n)
        fo = fanout.FanOut(dist, rank, world, nbranches, mine, src=0, device="cuda", always_broadcast=args.force_dist)
        # double-buffered: the broadcast of slab k+1 (communication stream) overlaps the branch kernels on slab k (FanOut.stream)
        import itertools
        slab_iter = fo.stream(itertools.repeat(x), 2 * n)
        last = {}

        def step():
            last.update(next(slab_iter))

        def outputs():
            return {"fanout_branch%d" % b: out.view(-1, 2) for b, out in sorted(last.items())}

        out_per_step = n
        alg_bytes = 9.6 * n
        flops = (4.0 * 128 / 5 + 6) * n
        config = {"workload": "configs[3]: one IQ slab of 2^%d samples broadcast from rank 0 (RCCL) to %d Tuner(offset_k, 100e3, 5) "
                              "branches, one per GPU" % (log2n, world),
                  "samples_per_step_per_gpu": n, "counted": "branch input samples", "parallelism": "fan-out x%d" % world}
        dominant = "fir_mfma_persistent_kernel<2,5,2,true,51>"

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # clock ramp: a GPU that has been idle runs its first ~100 ms of work well below the sustained clocks (measured on the gpurun
    # pool: 1.02 ms for the first timed FIR passes of a process, 0.85 ms from then on) - untimed, before the W warm-up steps
    if args.workload == "fanout" and (world > 1 or args.force_dist):
        for _ in range(8):            # a step holds a collective: every rank must run the SAME number of them (no time-based loop here)
            step()
        torch.cuda.synchronize()
    else:
        t_ramp = time.perf_counter()
        while time.perf_counter() - t_ramp < args.prewarm_ms / 1e3:
            for _ in range(4):
                step()
            torch.cuda.synchronize()
    # the ramp runs as many steps as the clock allows: a chain that carries state from step to step (rotator and decimation phase, filter
    # histories) starts again here, so that the timed steps compute the same output in every run with the same arguments
    if args.workload == "wbfm":
        rx.reset()
    elif args.workload == "fanout":
        for br in mine.values():
            br.block.reset()
    for _ in range(args.warmup):
        step()
    sync_all()
    timer = L.lrhip_timer_create()
    t0 = time.perf_counter()
    L.lrhip_timer_start(timer)
    for _ in range(args.steps):
        step()
    L.lrhip_timer_stop(timer)
    sync_all()
    wall = time.perf_counter() - t0
    ev_ms = L.lrhip_timer_elapsed_ms(timer)
    L.lrhip_timer_destroy(timer)
    dump = take_outputs(torch, outputs(), DUMP_BYTES // world) if args.dump_outputs else None
    # spread of the GPU figure (benchmarks/luaradio_benchmark.lua:10-13, 722-738: trials, mean and deviation): five more trials of the same K steps, each
    # between its own HIP event pair, AFTER the timed region above (which stays exactly K steps between two barriers) - and in the last of them every step
    # between its own pair, so that a 1-2 % change from one round to the next can be told from the spread of the box
    spread = None
    if world == 1:
        trial_ms = [ev_ms / args.steps]
        for _ in range(5):
            tt = L.lrhip_timer_create()
            L.lrhip_timer_start(tt)
            for _ in range(args.steps):
                step()
            L.lrhip_timer_stop(tt)
            trial_ms.append(L.lrhip_timer_elapsed_ms(tt) / args.steps)
            L.lrhip_timer_destroy(tt)
        step_timers = [L.lrhip_timer_create() for _ in range(args.steps)]
        for tt in step_timers:
            L.lrhip_timer_start(tt)
            step()
            L.lrhip_timer_stop(tt)
        torch.cuda.synchronize()
        step_ms = [L.lrhip_timer_elapsed_ms(tt) for tt in step_timers]
        for tt in step_timers:
            L.lrhip_timer_destroy(tt)

        def _stats(v):
            m = sum(v) / len(v)
            return {"mean": round(m, 4), "sigma": round((sum((a - m) ** 2 for a in v) / max(len(v) - 1, 1)) ** 0.5, 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}
        spread = {"trials_of_K_steps_ms_per_step": _stats(trial_ms), "single_steps_ms": _stats(step_ms),
                  "note": "HIP events on the launch stream; trial 1 is the timed region itself, trials 2-6 follow it; single steps: one event pair per step"}
    per_rank_wall = [wall]
    if dist is not None:
        cdev = dev if args.dist_backend == "nccl" else "cpu"
        mine_t = torch.tensor([wall], dtype=torch.float64, device=cdev)
        allw = [torch.zeros(1, dtype=torch.float64, device=cdev) for _ in range(world)]
        dist.all_gather(allw, mine_t)
        per_rank_wall = [float(w.item()) for w in allw]
        wall = max(per_rank_wall)

    rank_verified = None
    if args.workload == "timeshard" and not args.no_verify:
        ok, rms, worst = verify_partition(torch, dev, y, produced[-1], pa, pb, fs, -250e3)
        rank_verified = {"verified": ok, "rms_err_vs_oracle": rms, "max_err_vs_oracle": worst, "partition": [pa, pb]}
    elif args.workload == "fanout" and not args.no_verify:
        b0 = sorted(mine)[0]
        # one more (plain, in-place) broadcast leaves the slab in x on every rank; every rank checks its own branch against the oracle Tuner
        rv = verify_tuner_branch(torch, mine[b0].block, lambda: fo.push(x)[b0], x, n, fs, offs[b0 % len(offs)], 100e3, 5)
        rank_verified = {"verified": rv["verified"], "max_err_vs_oracle": rv["max_err_vs_oracle"], "branch": b0}
    if rank_verified is not None and dist is not None:
        gathered = [None] * world
        dist.all_gather_object(gathered, rank_verified)
        rank_verified = gathered
    elif rank_verified is not None:
        rank_verified = [rank_verified]

    verification = None
    if rank == 0 and world == 1 and args.workload == "fir" and not args.no_verify:
        verification = verify_fir_output(torch, x, y, n, taps, fir_mode)      # before the yardstick below reuses y

    # achievable-bandwidth yardstick on this box: the cheapest streaming kernel of the library (one multiply per scalar,
    # 8 B in + 8 B out per sample) over the same buffers, HIP-event timed like the workload
    yard_gbs = None
    if rank == 0 and args.workload == "fir":
        mc = lr.MultiplyConstantBlock(1.0)
        mc.differentiate([types.ComplexFloat32])
        mc.initialize()
        mc.process_device(x.data_ptr(), n, y.data_ptr(), n)
        yt = L.lrhip_timer_create()
        L.lrhip_timer_start(yt)
        for _ in range(5):
            mc.process_device(x.data_ptr(), n, y.data_ptr(), n)
        L.lrhip_timer_stop(yt)
        torch.cuda.synchronize()
        yard_gbs = 16.0 * n * 5 / (L.lrhip_timer_elapsed_ms(yt) / 1e3) / 1e9
        L.lrhip_timer_destroy(yt)

    if dump is not None:
        write_outputs(args.dump_outputs, dump, "rank%d_" % rank if world > 1 else "")

    if rank == 0:
        total = float(out_per_step) * world * args.steps
        launch_s = ev_ms / 1e3 / args.steps          # HIP-event time per step on the launch stream
        achieved = alg_bytes / launch_s / 1e9
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                ent = tj.get("%s:%d" % (args.workload if args.workload != "fir" else "fir-" + fir_mode, log2n))
                traffic = ent["bytes_per_launch"] if ent else None
            except Exception:
                traffic = None
        res = {
            "metric": "MSamples/s per block (128-tap complex FIR headline) + WBFM chain end-to-end",
            "value": round(total / wall / 1e6, 1), "unit": "MSamples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "prewarm_ms": args.prewarm_ms, "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": config,
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "kernel": dominant,
                         "algorithmic_bytes_per_launch": alg_bytes, "launch_ms_hip_events": round(launch_s * 1e3, 4),
                         "fp32_tflops": round(flops / launch_s / 1e12, 2), "fp32_peak_tflops": FP32_PEAK_TFLOPS,
                         "fp32_frac": round(flops / launch_s / 1e12 / FP32_PEAK_TFLOPS, 4)},
        }
        if spread is not None:
            res["ms_per_step_sigma"] = spread["trials_of_K_steps_ms_per_step"]["sigma"]
            res["ms_per_step_min"] = spread["trials_of_K_steps_ms_per_step"]["min"]
            res["ms_per_step_max"] = spread["trials_of_K_steps_ms_per_step"]["max"]
            res["spread"] = spread
        if args.workload == "timeshard":
            res["scaling"] = "strong"
        if rank_verified is not None:
            res["nranks"] = world
            res["verified"] = all(r["verified"] for r in rank_verified)
            res["per_rank_verified"] = rank_verified
        if dist is not None:
            res["dist_backend"] = args.dist_backend
        if args.workload == "fanout":
            # every receiving GPU takes the whole slab over ONE xGMI link from the source (point-to-point links, 7 x ~153 GB/s per GPU):
            # 8 B per ComplexFloat32 sample -> at most ~19.1 GS/s per receiver, far below what a branch filters (the fanout leg of the N = 1 line)
            res["fanout_links"] = {"per_rank_received_GB/s": [None if r == 0 else round(8.0 * n * args.steps / per_rank_wall[r] / 1e9, 1) for r in range(world)],
                                   "source_sent_GB/s": round(8.0 * n * args.steps * max(world - 1, 0) / wall / 1e9, 1),
                                   "xgmi_link_GB/s": 153.0, "xgmi_link_bound_MSps": 19125.0, "double_buffered": True,
                                   "note": "RCCL broadcast of each slab on a communication stream, overlapped with the branch kernels on the previous slab; "
                                           "a receiver is bounded by one link, so fan-out throughput is link-bound by construction"}
        if yard_gbs:
            res["roofline"]["streaming_yardstick"] = {"kernel": "multiply_constant_vec4_kernel<0> (MultiplyConstantBlock: 16 B per lane, one item per thread; 8 B in + 8 B out per sample, same buffers)",
                                                      "GB/s": round(yard_gbs, 1), "frac_of_yardstick": round(achieved / yard_gbs, 4)}
        if world == 1 and not args.no_cpu_baseline and args.workload == "fir":
            res["cpu_baseline"] = cpu_baseline_fir(taps, args.cpu_seconds)
        elif world == 1:
            res["cpu_baseline"] = None
        if verification:
            res.update(verification)
        if world == 1 and args.workload == "fir" and log2n >= 26 and not args.headline_only:
            del x, y
            torch.cuda.empty_cache()
            res["wbfm_chain"] = wbfm_chain_report(lr, L, torch, dev, not args.no_cpu_baseline)
            torch.cuda.empty_cache()
            res["channelizer"] = channelizer_report(lr, L, torch, dev, not args.no_cpu_baseline)
            torch.cuda.empty_cache()
            res["fanout"] = fanout_report(lr, L, torch, dev)
            torch.cuda.empty_cache()
            res["host_path"] = host_path_report(lr, L, torch, dev)
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
