#!/usr/bin/env python3
"""One shape of the polyphase + FFT channelizer alone (for the profiler): run_pfb_channelizer.py K M [steps [oversample]] - 2^24 samples per
step; oversample 2 or 4 runs the oversampled form (hop K / oversample).  With steps >= 100: 20 warm-up calls, then 5 windows of
`steps` calls, each between two events; prints the median window and every window in ms per step.  The file runs unchanged against an older
checkout of the package (copy it into that checkout's tools/), which is how the R = 1 kernel is compared across commits."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import luaradio_amd as lr
from luaradio_amd import types
lr.init(0)
lr.adopt_torch_stream()
K, M = int(sys.argv[1]), int(sys.argv[2])
n = 1 << 24
g = torch.Generator(device="cuda").manual_seed(5)
x = torch.rand(2 * n, dtype=torch.float32, device="cuda", generator=g) * 2 - 1
R = int(sys.argv[4]) if len(sys.argv) > 4 else 1
ch = lr.PolyphaseChannelizerBlock(K, lr.filter_utils.firwin_lowpass(M, 1.0 / K), {"method": "fft", "oversample": R} if R > 1 else {"method": "fft"})
ch.rate = 1102500.0
ch.differentiate([types.ComplexFloat32])
ch.initialize()
cap = ch.max_output(n)
y = torch.empty(2 * cap + 64, dtype=torch.float32, device="cuda")
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
for _ in range(20 if steps >= 100 else 1):
    ch.process_device(x.data_ptr(), n, y.data_ptr(), cap)
torch.cuda.synchronize()
windows = []
for _ in range(5 if steps >= 100 else 1):          # a profiler run asks for a few steps and gets exactly those
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        ch.process_device(x.data_ptr(), n, y.data_ptr(), cap)
    t1.record()
    torch.cuda.synchronize()
    windows.append(t0.elapsed_time(t1) / steps)
print("ok K=%d M=%d R=%d ms_per_step median %.4f windows %s" % (K, M, R, sorted(windows)[len(windows) // 2], " ".join("%.4f" % w for w in windows)))
