#!/usr/bin/env python3
"""Wideband FM broadcast (stereo) receiver from an IQ recording into a two-channel WAV file - the reference's
examples/rtlsdr_wbfm_stereo.lua with the RTL-SDR source replaced by IQFileSource and its audio sink by WAVFileSink(path, 2):

    IQFileSource(file, 'u8', 1102500) -> wbfm_stereo_receiver (Tuner, discriminator, pilot PLL, L+R / L-R, de-emphasis, Downsampler(5))
        -> WAVFileSink(path, 2): left and right are interleaved and quantised to s16le in one pass on the device

IQ records come in and interleaved PCM records go out; the float channels stay on the device.

    python examples/iqfile_wbfm_stereo.py capture.u8 out.wav [--format u8] [--rate 1102500] [--offset -250e3] [--bits 16]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import luaradio_amd as lr                     # noqa: E402


def build_graph(rate, offset, wav_path, bits):
    """the receiver's graph with its two audio outputs connected to the sink's in1 / in2"""
    g = lr.wbfm_stereo_receiver(rate, offset)
    left = next(n.block for n in g._order if n.block.name == "left")
    right = next(n.block for n in g._order if n.block.name == "right")
    sink = lr.WAVFileSink(wav_path, 2, bits)
    g.connect(left, "out", sink, "in1")
    g.connect(right, "out", sink, "in2")
    return g.initialize(), sink


def run(src, g, sink, records_per_call=1 << 20):
    """chunks of the file (8192 records each, as the reference reads them) gathered into calls of records_per_call samples"""
    import numpy as np
    pending, have = [], 0
    while True:
        x = src.process()
        if x is not None:
            pending.append(x)
            have += len(x)
        if pending and (x is None or have >= records_per_call):
            g.process(**{"in": np.concatenate(pending)})
            pending, have = [], 0
        if x is None:
            break
    sink.cleanup()
    return sink.num_samples


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("capture")
    ap.add_argument("wav")
    ap.add_argument("--format", default="u8")
    ap.add_argument("--rate", type=float, default=1102500.0)
    ap.add_argument("--offset", type=float, default=-250e3)
    ap.add_argument("--bits", type=int, default=16, choices=(8, 16, 32))
    a = ap.parse_args()
    lr.init()
    src = lr.IQFileSource(a.capture, a.format, a.rate)
    src.initialize()
    g, sink = build_graph(a.rate, a.offset, a.wav, a.bits)
    frames = run(src, g, sink)
    src.cleanup()
    print("%s: %d frames of 2 x %d bits at %g Hz" % (a.wav, frames, a.bits, sink.get_rate()))


if __name__ == "__main__":
    main()
