"""File sources feeding the device path - mirrors radio/blocks/sources/iqfile.lua and realfile.lua.

The file is read on the host in the reference's chunks (8192 samples, iqfile.lua:52); the RAW records are handed to
the device unchanged and converted there ((value - offset)/scale after the byte swap, format_utils.lua:82-97), so
an RTL-SDR style `u8` capture crosses PCIe at 2 bytes per complex sample instead of 8.
"""
import ctypes as C
import io
import struct

import numpy as np

from . import _lib, types
from .block import Block, Input, Output
from .blocks import _PortBlock, _Scratch

# radio/utilities/format_utils.lua:82-97 (bytes per raw scalar)
FORMAT_BYTES = {"u8": 1, "s8": 1, "u16le": 2, "u16be": 2, "s16le": 2, "s16be": 2, "u32le": 4, "u32be": 4,
                "s32le": 4, "s32be": 4, "f32le": 4, "f32be": 4, "f64le": 8, "f64be": 8}


class _FileSource(Block):
    _complex = True

    def instantiate(self, file, format, rate, repeat_on_eof=False):
        assert file is not None, "Missing argument #1 (file)"
        assert format, "Missing argument #2 (format)"
        if format not in FORMAT_BYTES:
            raise AssertionError('Unsupported format ("%s")' % format)       # iqfile.lua:48
        assert rate, "Missing argument #3 (rate)"
        self.file, self.format, self.rate = file, format, rate
        self.repeat_on_eof = repeat_on_eof or False
        self.chunk_size = 8192
        self.record_size = FORMAT_BYTES[format] * (2 if self._complex else 1)
        out_type = types.ComplexFloat32 if self._complex else types.Float32
        self.add_type_signature([], [Output("out", out_type)])
        self.signature = self.type_signatures[0]

    def get_rate(self):
        return self.rate

    def initialize(self):
        if isinstance(self.file, (bytes, bytearray)):
            self._fh = io.BytesIO(bytes(self.file))          # tests/buffer.lua: an in-memory file
        elif isinstance(self.file, str):
            self._fh = open(self.file, "rb")
        else:
            self._fh = self.file
        self._set_stage(_lib.load().lrhip_format_convert_create(self.format.encode(), int(self._complex)),
                        "Creating lrhip format object")

    def process(self):
        """One chunk, or None at end of file (iqfile.lua:82-96)."""
        raw = self._fh.read(self.chunk_size * self.record_size)
        num_samples = len(raw) // self.record_size
        if num_samples == 0 and self.repeat_on_eof:
            self._fh.seek(0)                  # iqfile.lua:86-90: rewind once and read again; a file without one whole record still ends
            raw = self._fh.read(self.chunk_size * self.record_size)
            num_samples = len(raw) // self.record_size
        if num_samples == 0:
            return None
        L = _lib.load()
        buf = np.frombuffer(raw, dtype=np.uint8, count=num_samples * self.record_size)
        out = np.empty(num_samples, dtype=self.get_output_type().dtype)
        n = L.lrhip_stage_execute(self._stage, buf.ctypes.data_as(C.c_void_p), num_samples, out.ctypes.data_as(C.c_void_p), num_samples)
        _lib.check(n, "%s:process" % self.name)
        return out

    def read_all(self):
        """Convenience: the whole file as one vector (chunks concatenated)."""
        parts = []
        while True:
            v = self.process()
            if v is None:
                break
            parts.append(v)
        return np.concatenate(parts) if parts else np.zeros(0, self.get_output_type().dtype)

    def cleanup(self):
        if isinstance(self.file, str):
            self._fh.close()


class IQFileSource(_FileSource):
    """radio/blocks/sources/iqfile.lua. IQFileSource(file, format, rate[, repeat_on_eof])."""
    name = "IQFileSource"
    _complex = True


class RealFileSource(_FileSource):
    """radio/blocks/sources/realfile.lua. RealFileSource(file, format, rate[, repeat_on_eof])."""
    name = "RealFileSource"
    _complex = False


class _FileSink(Block):
    """radio/blocks/sinks/iqfile.lua / realfile.lua: samples -> raw records on the device, written by the host."""
    _complex = True

    def instantiate(self, file, format):
        assert file is not None, "Missing argument #1 (file)"
        assert format, "Missing argument #2 (format)"
        if format not in FORMAT_BYTES:
            raise AssertionError('Unsupported format ("%s")' % format)
        self.file, self.format = file, format
        self.record_size = FORMAT_BYTES[format] * (2 if self._complex else 1)
        self.add_type_signature([Input("in", types.ComplexFloat32 if self._complex else types.Float32)], [])

    def initialize(self):
        self._fh = open(self.file, "wb") if isinstance(self.file, str) else self.file
        self._set_stage(_lib.load().lrhip_format_pack_create(self.format.encode(), int(self._complex)), "Creating lrhip format object")

    def process(self, x):
        x = np.ascontiguousarray(x, dtype=self.get_input_type().dtype)
        out = np.empty(len(x) * self.record_size, np.uint8)
        n = _lib.load().lrhip_stage_execute(self._stage, x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), len(x))
        _lib.check(n, "%s:process" % self.name)
        self._fh.write(out.tobytes())

    def cleanup(self):
        if isinstance(self.file, str):
            self._fh.close()
        else:
            self._fh.flush()


class IQFileSink(_FileSink):
    """radio/blocks/sinks/iqfile.lua. IQFileSink(file, format)."""
    name = "IQFileSink"
    _complex = True


class RealFileSink(_FileSink):
    """radio/blocks/sinks/realfile.lua. RealFileSink(file, format)."""
    name = "RealFileSink"
    _complex = False


# ---- WAV files (radio/blocks/sinks/wavfile.lua, radio/blocks/sources/wavfile.lua): a 44-byte header and records of num_channels raw samples,
# packed / unpacked on the device in the same pass that interleaves / deinterleaves them ("wavpack" / "wavunpack", csrc/stage_interleave.h)
WAV_FORMATS = {8: "u8", 16: "s16le", 32: "s32le"}          # wavfile.lua:59-63
WAV_HEADER_SIZE = 44
_WAV_HEADER = struct.Struct("<4sI4s4sIHHIIHH4sI")          # riff_header_t, wave_subchunk1_header_t, wave_subchunk2_header_t


def wav_header(rate, num_channels, bits_per_sample, num_frames):
    """the 44 header bytes WAVFileSink:cleanup() writes after num_frames samples per channel (sinks/wavfile.lua:141-155, :203-205); the
    sizes wrap modulo 2^32 as the reference's uint32_t fields do"""
    u32 = 0xFFFFFFFF
    sample_bytes = bits_per_sample // 8
    data_size = (num_frames * num_channels * sample_bytes) & u32
    return _WAV_HEADER.pack(b"RIFF", (4 + (8 + 16) + (8 + data_size)) & u32, b"WAVE", b"fmt ", 16, 1, num_channels, int(rate) & u32,
                            int(rate * num_channels * sample_bytes) & u32, (num_channels * sample_bytes) & 0xFFFF, bits_per_sample, b"data", data_size)


def parse_wav_header(header, num_channels=None):
    """(rate, num_channels, bits_per_sample) of a 44-byte header, with the checks and messages of sources/wavfile.lua:162-187, in their order;
    num_channels: the block's channel count, which the file must match"""
    if len(header) < WAV_HEADER_SIZE:
        raise ValueError("Invalid WAV file: header of %d bytes, expected %d." % (len(header), WAV_HEADER_SIZE))
    riff_id, _, riff_format, fmt_id, _, audio_format, channels, rate, _, _, bits, data_id, _ = _WAV_HEADER.unpack(bytes(header[:WAV_HEADER_SIZE]))
    if riff_id != b"RIFF":
        raise ValueError("Invalid WAV file: invalid RIFF header id.")
    if riff_format != b"WAVE":
        raise ValueError("Invalid WAV file: invalid RIFF header format.")
    if fmt_id != b"fmt ":
        raise ValueError("Invalid WAV file: invalid WAVE subchunk1 header id.")
    if audio_format != 1:
        raise ValueError("Unsupported WAV file: unsupported audio format %d (not PCM)." % audio_format)
    if num_channels is not None and channels != num_channels:
        raise ValueError("Block number of channels (%d) does not match WAV file number of channels (%d)." % (num_channels, channels))
    if bits not in WAV_FORMATS:
        raise ValueError("Unsupported WAV file: unsupported bits per sample %d." % bits)
    if data_id != b"data":
        raise ValueError("Invalid WAV file: invalid WAVE subchunk2 header id.")
    return rate, channels, bits


def wav_chunk_samples(num_channels, chunk_size=8192):
    """raw samples WAVFileSource reads per chunk: the reference's 8192 where whole frames fill it, otherwise the whole frames inside it.  (The
    reference reads 8192 there as well and converts 8192 / N frames with a fractional loop bound: 8192 mod N samples are lost per chunk and the
    channels rotate from chunk to chunk - DESIGN.md section 8.)"""
    return chunk_size if chunk_size % num_channels == 0 else chunk_size // num_channels * num_channels


def wav_op(name, num_channels, bits_per_sample):
    return "%s:channels=%d:bits=%d" % (name, num_channels, bits_per_sample)


def _wav_ports(kind, num_channels):
    if num_channels == 1:
        return [kind("in" if kind is Input else "out", types.Float32)]
    return [kind("%s%d" % ("in" if kind is Input else "out", i + 1), types.Float32) for i in range(num_channels)]


class WAVFileSink(_PortBlock):
    """radio/blocks/sinks/wavfile.lua. WAVFileSink(file, num_channels[, bits_per_sample=16]): in1 .. inN Float32 (N = 1: in) -> a PCM WAV
    file of 8, 16 or 32 bits per sample.  `file` is a path or a seekable file object: a placeholder header goes first, then the records,
    and cleanup() rewrites the header with the sizes."""
    name = "WAVFileSink"

    def instantiate(self, file, num_channels, bits_per_sample=16):
        assert file is not None, "Missing argument #1 (file)"
        assert num_channels is not None, "Missing argument #2 (num_channels)"
        self.file, self.num_channels = file, num_channels
        self.bits_per_sample = 16 if bits_per_sample is None else bits_per_sample
        if self.bits_per_sample not in WAV_FORMATS:
            raise AssertionError("Unsupported bits per sample (%s)" % (bits_per_sample,))       # wavfile.lua:76
        assert isinstance(num_channels, int) and 1 <= num_channels <= _lib.MAX_PORTS, "Number of channels must be 1 .. %d" % _lib.MAX_PORTS
        self.format = WAV_FORMATS[self.bits_per_sample]
        self.record_size = num_channels * self.bits_per_sample // 8
        self.num_samples = 0
        self.add_type_signature(_wav_ports(Input, num_channels), [])

    def op(self):
        return wav_op("wavpack", self.num_channels, self.bits_per_sample)

    def initialize(self):
        self._fh = open(self.file, "wb") if isinstance(self.file, str) else self.file
        if not self._fh.seekable():
            raise ValueError("WAVFileSink needs a path or a seekable file object: the header is rewritten in cleanup()")
        self._start = self._fh.tell()
        self._fh.write(bytes(WAV_HEADER_SIZE))
        self.num_samples = 0
        self._create(self.op())

    def write_device(self, in_ptrs, n):
        """n samples per channel from the device vectors in_ptrs: packed into a device record buffer, copied down and written"""
        if not n:
            return
        with _Scratch() as s:
            rec = s.alloc(n * self.record_size)
            got = self.process_device_ports(list(in_ptrs), n, [rec], n)
            self._fh.write(s.download(rec, got * self.record_size, np.uint8).tobytes())
        self.num_samples += n

    def process(self, *xs):
        xs = self._same_length(xs, np.float32)
        with _Scratch() as s:
            self.write_device([s.upload(x) for x in xs], len(xs[0]))

    def cleanup(self):
        end = self._fh.tell()
        self._fh.seek(self._start)
        self._fh.write(wav_header(self.get_rate(), self.num_channels, self.bits_per_sample, self.num_samples))
        self._fh.seek(end)
        if isinstance(self.file, str):
            self._fh.close()
        else:
            self._fh.flush()


class WAVFileSource(_PortBlock):
    """radio/blocks/sources/wavfile.lua. WAVFileSource(file, num_channels[, repeat_on_eof=False]): a PCM WAV file of 8, 16 or 32 bits per
    sample -> out1 .. outN Float32 (N = 1: out) at the file's sample rate.  `file` is a path, a file object or bytes.  process() returns one
    chunk - a tuple of N vectors, a single vector for N = 1 - or None at the end of the file."""
    name = "WAVFileSource"
    _many_in = False

    def instantiate(self, file, num_channels, repeat_on_eof=False):
        assert file is not None, "Missing argument #1 (file)"
        assert num_channels is not None, "Missing argument #2 (num_channels)"
        assert isinstance(num_channels, int) and 1 <= num_channels <= _lib.MAX_PORTS, "Number of channels must be 1 .. %d" % _lib.MAX_PORTS
        self.file, self.num_channels = file, num_channels
        self.repeat_on_eof = repeat_on_eof or False
        self.rate = None
        self.chunk_size = 8192
        self.add_type_signature([], _wav_ports(Output, num_channels))
        self.signature = self.type_signatures[0]

    def get_rate(self):
        return self.rate or 1           # wavfile.lua:93-95

    def op(self):
        return wav_op("wavunpack", self.num_channels, self.bits_per_sample)

    def initialize(self):
        if isinstance(self.file, (bytes, bytearray)):
            self._fh = io.BytesIO(bytes(self.file))
        elif isinstance(self.file, str):
            self._fh = open(self.file, "rb")
        else:
            self._fh = self.file
        self._data_start = None
        header = self._fh.read(WAV_HEADER_SIZE)
        self.rate, _, self.bits_per_sample = parse_wav_header(header, self.num_channels)
        self.format = WAV_FORMATS[self.bits_per_sample]
        self.record_size = self.num_channels * self.bits_per_sample // 8
        self._create(self.op())

    def _read_chunk(self):
        raw = self._fh.read(wav_chunk_samples(self.num_channels, self.chunk_size) * (self.bits_per_sample // 8))
        return raw, len(raw) // self.record_size

    def process(self):
        raw, frames = self._read_chunk()
        if frames == 0 and self.repeat_on_eof:
            self._fh.seek(WAV_HEADER_SIZE)          # wavfile.lua:209-214: rewind past the header
            raw, frames = self._read_chunk()
        if frames == 0:
            return None
        buf = np.frombuffer(raw, np.uint8, frames * self.record_size)
        with _Scratch() as s:
            outs = [s.alloc(frames * 4) for _ in range(self.num_channels)]
            got = self.process_device_ports([s.upload(buf)], frames, outs, frames)
            ys = tuple(s.download(p, got, np.float32) for p in outs)
        return ys[0] if self.num_channels == 1 else ys

    def read_all(self):
        """Convenience: the whole file, chunks concatenated (a tuple of N vectors, a single vector for N = 1)."""
        parts = []
        while True:
            v = self.process()
            if v is None:
                break
            parts.append((v,) if self.num_channels == 1 else v)
        ys = tuple(np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, np.float32) for k in range(self.num_channels))
        return ys[0] if self.num_channels == 1 else ys

    def cleanup(self):
        if isinstance(self.file, str):
            self._fh.close()


# ---- generator sources (csrc/stage_source.h): no input, sample n a closed form of the absolute index n -------------------------------------
SIGNALS = {"exponential": types.ComplexFloat32, "cosine": types.Float32, "sine": types.Float32, "square": types.Float32,
           "triangle": types.Float32, "sawtooth": types.Float32, "constant": types.Float32}          # signal.lua:40-48


def signal_op(signal, frequency, rate, amplitude=1.0, phase=0.0, offset=0.0):
    return "signalsource:signal=%s:frequency=%.17g:rate=%.17g:amplitude=%.17g:phase=%.17g:offset=%.17g" % (
        signal, float(frequency), float(rate), float(amplitude), float(phase), float(offset))


def uniform_random_op(type_name, lo, hi, seed):
    return "uniformrandomsource:type=%s:lo=%.17g:hi=%.17g:seed=%d" % (type_name, float(lo), float(hi), int(seed))


class _GeneratorSource(Block):
    """a block whose stage has no input: process(n) generates the next n samples of the stream, seek(n0) moves to absolute sample n0"""
    is_source = True

    def op(self):
        raise NotImplementedError

    def get_rate(self):
        return self.rate

    def initialize(self):
        self._set_stage(_lib.load().lrhip_unary_create(self.op().encode(), 0.0, 0.0, 0, 0), "Creating lrhip %s object" % self.op().split(":")[0])

    def process(self, n=None):
        """the next n samples (chunk_size when n is None, the reference's chunk)"""
        n = self.chunk_size if n is None else int(n)
        out = np.empty(n, dtype=self.get_output_type().dtype)
        got = _lib.load().lrhip_stage_execute(self.stage_handle(), None, n, out.ctypes.data_as(C.c_void_p), n)
        _lib.check(got, "%s:process" % self.name)
        return out[:got]

    def process_device(self, out_ptr, n):
        """the next n samples into device memory at out_ptr, asynchronous on the library stream"""
        got = _lib.load().lrhip_stage_execute_device(self.stage_handle(), None, int(n), out_ptr, int(n))
        return _lib.check(got, "%s:process_device" % self.name)


class SignalSource(_GeneratorSource):
    """radio/blocks/sources/signal.lua. SignalSource(signal, frequency, rate[, {amplitude=1, offset=0, phase=0}]): "exponential" gives
    ComplexFloat32, "cosine", "sine", "square", "triangle", "sawtooth" and "constant" Float32.  The reference adds omega to a running double phase
    and wraps it once per chunk; here the phase of sample n is n * frequency / rate + phase / 2 pi turns in exact 64-bit fixed point, so any chunking
    gives the same bits and seek(n0) continues at sample n0 (include/lrhip.h has the closed forms)."""
    name = "SignalSource"

    def instantiate(self, signal=None, frequency=None, rate=None, options=None):
        assert signal, "Missing argument #1 (signal)"
        if signal not in SIGNALS:
            raise AssertionError('Unsupported signal ("%s")' % (signal,))          # signal.lua:50
        assert frequency is not None, "Missing argument #2 (frequency)"
        assert rate, "Missing argument #3 (rate)"
        self.signal, self.frequency, self.rate = signal, frequency, rate
        self.options = dict(options or {})
        self.chunk_size = 8192
        self.add_type_signature([], [Output("out", SIGNALS[signal])])
        self.signature = self.type_signatures[0]

    def op(self):
        o = self.options
        return signal_op(self.signal, self.frequency, self.rate, 1.0 if o.get("amplitude") is None else o["amplitude"],
                         o.get("phase") or 0.0, o.get("offset") or 0.0)


_RANDOM_TYPES = {types.ComplexFloat32: "cf32", types.Float32: "f32", types.Byte: "byte", types.Bit: "bit"}


class UniformRandomSource(_GeneratorSource):
    """radio/blocks/sources/uniformrandom.lua. UniformRandomSource(data_type, rate[, {lo, hi}[, {seed=}]]): ComplexFloat32, Float32, Byte or Bit
    samples drawn uniformly from [lo, hi] - [-1, 1] by default for the float types, [0, 255] for Byte (integers; the reference's own Byte default is
    broken: `a = a or 0, b or 255` at uniformrandom.lua:56 leaves b nil), always {0, 1} for Bit.  The reference draws from LuaJIT's sequential
    math.random; here word j of the stream is Philox4x32-10 of the absolute index and the seed (0 when none is given: the reference without a seed is
    deterministic per run too), so the contract is distribution, range and determinism per seed, not LuaJIT's values, and any chunking or seek(n0)
    gives the same bits."""
    name = "UniformRandomSource"

    def instantiate(self, data_type=None, rate=None, range=None, options=None):
        assert data_type is not None, "Missing argument #1 (data_type)"
        assert rate, "Missing argument #2 (rate)"
        assert any(data_type is t for t in _RANDOM_TYPES), "Unsupported data type"          # uniformrandom.lua:73
        self.data_type, self.rate = data_type, rate
        lo, hi = (list(range or []) + [None, None])[:2]
        if data_type is types.Byte:
            lo, hi = 0 if lo is None else lo, 255 if hi is None else hi
        elif data_type is types.Bit:
            lo, hi = 0, 1
        else:
            lo, hi = -1.0 if lo is None else lo, 1.0 if hi is None else hi
        self.range = (lo, hi)
        seed = (options or {}).get("seed")
        self.seed = 0 if seed is None else int(seed)
        assert 0 <= self.seed < 1 << 64, "seed must be an integer in 0 .. 2^64 - 1"
        self.chunk_size = 8192
        self.add_type_signature([], [Output("out", data_type)])
        self.signature = self.type_signatures[0]

    def op(self):
        return uniform_random_op(_RANDOM_TYPES[self.data_type], self.range[0], self.range[1], self.seed)
