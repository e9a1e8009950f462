#!/usr/bin/env python3
"""One shape of the polyphase + FFT channelizer alone (for the profiler): run_pfb_channelizer.py K M [steps] - 2^24 samples per step"""
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
ch = lr.PolyphaseChannelizerBlock(K, lr.filter_utils.firwin_lowpass(M, 1.0 / K), {"method": "fft"})
ch.rate = 1102500.0
ch.differentiate([types.ComplexFloat32])
ch.initialize()
cap = ch.max_output(n)
y = torch.empty(2 * cap + 64, dtype=torch.float32, device="cuda")
for _ in range(int(sys.argv[3]) if len(sys.argv) > 3 else 10):
    ch.process_device(x.data_ptr(), n, y.data_ptr(), cap)
torch.cuda.synchronize()
print("ok")
