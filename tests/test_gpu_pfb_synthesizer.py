"""PolyphaseSynthesizerBlock (pfb_synth_ifft_kernel + pfb_synth_sums_kernel, kernels_pfbsynth.h: K channels, frame hop D = K / R) through the C ABI
against the float64 filterbank of tests/helpers/synthesizer_ref.py over every tiling class, and the promises that do not depend on rounding: an
output is a pure function of the Q frames under its taps, so every chunking and every entry path gives the same bytes; a frame reaches exactly
the outputs under its M taps; a call writes exactly its outputs; reset() forgets the partial frame, the history and the class; and behind the
oversampled analysis bank the block gives the input back.

Bars: per output and component (2 K Q + 2) 2^-24 B[n] (the worst case of direct summation; a gross-error catch), and over all outputs
rms(|got - ref| / (2^-24 B[n])) <= 3 x the same figure of synthesize_f32_emulation on the same inputs (the device's radix-4 Stockham order and
its fmaf chain round differently from the emulation's transform, not worse)."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, filter_utils, types
from oracle import oracle as O
from tests.helpers import guarded as GD
from tests.helpers import synthesizer_ref as SR

pytestmark = pytest.mark.gpu


def tile_frames(K, R):
    """frames per workgroup of the larger-tiled of the two kernels (PfbSynthesizerStage::ifft_tile, sums_tile); only sizes the streams"""
    ifft = 2048 // K if K <= 256 else 8 if K == 512 else 4 if K == 1024 else 8192 // K
    sums = R * (8 if R == 1 else 4) * max(1, 512 // K)
    return max(ifft, sums)


def make(K, taps, R):
    blk = lr.PolyphaseSynthesizerBlock(K, taps, {"oversample": R})
    blk.rate = 2.0
    blk.differentiate([types.ComplexFloat32])
    blk.initialize()
    return blk


def make_analysis(K, taps, R):
    blk = lr.PolyphaseChannelizerBlock(K, taps, {"method": "fft"} if R == 1 else {"oversample": R})
    blk.rate = 2.0
    blk.differentiate([types.ComplexFloat32])
    blk.initialize()
    return blk


def rand_c(rng, n, scale=1.0):
    return (scale * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))).astype(np.complex64)


def prototype(kind, M, K, rng):
    if kind == "lowpass":
        return O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    return rng.uniform(-1, 1, M).astype(np.float32)          # non-symmetric, no near-zero edge taps


def run_host(blk, y, cuts=()):
    """process() over the flat frame stream y cut at the given positions; returns (outputs, outputs per call)"""
    parts, a = [], 0
    for b in list(cuts) + [len(y)]:
        parts.append(blk.process(y[a:b]))
        a = b
    return np.concatenate(parts), [len(p) for p in parts]


def bars(got, y, h, K, R, tag):
    """both bars against float64 for the frames y; the aggregate one from the Float32 emulation on the same inputs"""
    D = K // R
    Q = (len(h) + D - 1) // D
    ref, B = SR.synthesize_f64(y, h, K, R)
    emu = SR.rms_ratio(SR.synthesize_f32_emulation(y, h, K, R), ref, B)
    r = SR.check_bars(got, ref, B, K, Q, 3 * emu)
    print("synthesizer error ratio %s K=%d M=%d R=%d: device rms %.4f max %.4f, emulation rms %.4f (per-output bar %d)"
          % (tag, K, len(h), R, r, float(np.max(SR.error_ratio(got, ref, B))), emu, 2 * K * Q + 2))
    return r


class DeviceStream:
    """the whole frame stream resident on the device, `offset` complex64 values past a 16-byte boundary; calls are slices of it (process_device)
    and their outputs land back to back, `offset` samples past a 16-byte boundary as well"""

    def __init__(self, blk, y, K, D, offset=0):
        import torch
        self.torch, self.blk, self.offset = torch, blk, offset
        self.xd = torch.from_numpy(np.concatenate([np.zeros(offset, np.complex64), y]).view(np.float32)).cuda()
        self.cap = (len(y) // K + 1) * D
        self.yd = torch.empty(2 * (offset + self.cap), dtype=torch.float32, device="cuda")
        self.done = 0
        torch.cuda.synchronize()

    def call(self, a, b):
        got = self.blk.process_device(self.xd.data_ptr() + 8 * (self.offset + a), b - a, self.yd.data_ptr() + 8 * (self.offset + self.done), self.cap - self.done)
        _lib.load().lrhip_synchronize()
        self.done += got
        return got

    def result(self):
        self.torch.cuda.synchronize()
        return self.yd[2 * self.offset:2 * (self.offset + self.done)].cpu().numpy().view(np.complex64)


def test_the_block_is_the_stage():
    """max_output(n) = ceil(n / K) D, 8-byte samples on both sides, get_rate() = rate / R, process() of (frames, K) and of the flat stream; a
    partial frame waits for the next call; seek is refused"""
    L = _lib.load()
    rng = np.random.default_rng(1)
    for R, D in ((1, 64), (2, 32), (4, 16)):
        blk = make(64, np.ones(1024, np.float32), R)
        for n in (0, 1, 63, 64, 65, 640, 641):
            assert L.lrhip_stage_max_output(blk._stage, n) == (n + 63) // 64 * D
        assert L.lrhip_stage_input_size(blk._stage) == 8 and L.lrhip_stage_output_size(blk._stage) == 8
        assert blk.get_rate() == 2.0 / R
        y = rand_c(rng, 10 * 64 + 1)
        got = blk.process(y[:640].reshape(10, 64))
        assert got.shape == (10 * D,) and got.dtype == np.complex64
        assert len(blk.process(y[640:])) == 0 and len(blk.process(y[:62])) == 0 and len(blk.process(y[:1])) == D
        flat = make(64, np.ones(1024, np.float32), R).process(y[:640])
        assert flat.tobytes() == got.tobytes()
    with pytest.raises(Exception):
        blk.seek(64)


SHAPES = [(K, M, R) for K in (8, 16, 64, 256, 512, 1024, 2048, 4096) for M in (K, K + 1, 3 * K - 1, 16 * K) for R in (1, 2, 4)]


@pytest.mark.parametrize("K,M,R", SHAPES)
def test_shape_matrix_vs_f64(K, M, R):
    """3 whole tiles and a partial one (T // 2 + 1 frames) over two calls; the first call ends 3 values into a frame after T + T // 2 frames (not
    a multiple of R where T > 2), so the second starts on the carried partial frame, on a class other than 0, and reads the V history; a Hamming
    lowpass and random taps, random frames"""
    rng = np.random.default_rng(K * 10007 + M + R)
    D = K // R
    T = tile_frames(K, R)
    F = 3 * T + T // 2 + 1
    c1 = T + T // 2 + (1 if R > 1 and (T + T // 2) % R == 0 else 0)
    cut = c1 * K + 3
    for kind in ("lowpass", "random"):
        h = prototype(kind, M, K, rng)
        y = rand_c(rng, F * K)
        got, per_call = run_host(make(K, h, R), y, [cut])
        assert per_call == [c1 * D, (F - c1) * D]
        bars(got, y, h, K, R, kind)


@pytest.mark.parametrize("K,M,R", [(8, 23, 4), (64, 1000, 2), (512, 32768, 2), (2048, 2049, 4), (4096, 65536, 1)])
def test_chunking_is_bit_invariant(K, M, R):
    """one call and ragged chunkings give identical bytes: calls of 0, 1, K - 1, K and K + 1 values, calls that complete no frame, calls of
    fewer frames than the history holds (the carried rows move through the transit buffer) and calls of several tiles (interior workgroups take
    the unchecked load path); host process() pieces, and process_device slices of a resident stream 0 and 1 values past a 16-byte boundary"""
    rng = np.random.default_rng(K + 3 * M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    T = tile_frames(K, R)
    Q = (M + D - 1) // D
    big = (3 * T + 2) * K + 5
    small = [1, 0, K - 1, K, K + 1, 3, 1, K - 2, 2, 2 * K + 7, K // 2, K // 2 - 1]
    lens = small + [big, big + 1, 2 * K + 1, 0, (Q + 3) * K + 3, 1, 1, K - 1, big // 2, 5 * K + 3]
    n = sum(lens) // K * K
    lens[-1] -= sum(lens) - n                                  # the stream ends on a frame, so that every value is used
    assert lens[-1] > 0
    y = rand_c(rng, n)
    whole, _ = run_host(make(K, h, R), y)
    assert len(whole) == n // K * D
    bars(whole, y, h, K, R, "one call")

    cuts = [int(c) for c in np.cumsum(lens)[:-1]]
    got, per_call = run_host(make(K, h, R), y, cuts)
    assert per_call.count(0) >= 4, per_call
    assert got.tobytes() == whole.tobytes()

    edges = [0] + cuts + [n]
    for offset in (0, 1):
        ds = DeviceStream(make(K, h, R), y, K, D, offset)
        zero = sum(ds.call(a, b) == 0 for a, b in zip(edges[:-1], edges[1:]))
        assert zero >= 4
        assert ds.result().tobytes() == whole.tobytes(), offset


@pytest.mark.parametrize("R", [1, 2, 4])
def test_a_cut_on_every_residue(R):
    """K = 16, M = 50: the stream cut after 5 K + j values for every j < K (every length of the carried partial frame), and into calls of j + 1
    values throughout"""
    K, M = 16, 50
    rng = np.random.default_rng(16050 + R)
    h = prototype("random", M, K, rng)
    n = 40 * K
    y = rand_c(rng, n)
    whole, _ = run_host(make(K, h, R), y)
    bars(whole, y, h, K, R, "one call")
    for j in range(K):
        got, _ = run_host(make(K, h, R), y, [5 * K + j])
        assert got.tobytes() == whole.tobytes(), j
        got, _ = run_host(make(K, h, R), y, list(range(j + 1, n, j + 1)))
        assert got.tobytes() == whole.tobytes(), j


@pytest.mark.parametrize("K,M,R", [(8, 27, 4), (64, 1000, 2), (1024, 2500, 2), (4096, 9000, 4)])
def test_footprint(K, M, R):
    """a NaN (real part), and separately an Inf (imaginary part), in one value of frame s: exactly the outputs s D .. s D + M - 1 are non-finite
    (either component: with real taps a column of V may carry the value in one component only), every other output is finite.  M is not a
    multiple of D, so the last tap row is partly padding: an output whose padded row covers frame s but whose M taps do not must stay finite.
    s lies in the first call, so part of every footprint comes from the carried history (or, for the frame the cut falls in, the carried
    partial frame) in the second"""
    rng = np.random.default_rng(5 * K + M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    T = tile_frames(K, R)
    Q = (M + D - 1) // D
    F1 = T + 3
    F = F1 + 2 * T + Q + 2
    cut = F1 * K + K // 2 + 1                                 # frame F1 is the partial frame of call 1
    base = rand_c(rng, F * K)
    n = np.arange(F * D)
    cases = {"first frame": (0, 0), "last whole frame of call 1": (F1 - 1, K - 1), "partial frame, sent in call 1": (F1, K // 2),
             "Q - 2 frames before the partial one": (max(0, F1 - Q + 2), 1), "interior of call 1": (F1 // 2, K // 3)}
    for name, (s, c) in cases.items():
        assert s * K + c < cut
        for v in (np.nan, np.inf):
            y = base.copy()
            y[s * K + c] = complex(v, 0) if np.isnan(v) else complex(0, v)
            got, _ = run_host(make(K, h, R), y, [cut])
            assert got.shape == (F * D,)
            hit = (s * D <= n) & (n <= s * D + M - 1)
            assert hit.sum() == M
            nonfin = ~(np.isfinite(got.real) & np.isfinite(got.imag))
            assert nonfin[hit].all(), (name, s, v, np.flatnonzero(hit & ~nonfin)[:4])
            assert not nonfin[~hit].any(), (name, s, v, np.flatnonzero(nonfin & ~hit)[:4])


class TorchMemory:
    """device allocations through torch; an address is data_ptr() + byte offset (the memory interface of tests/helpers/guarded.py)"""

    def __init__(self):
        import torch
        self.torch = torch

    def alloc(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda")

    def write(self, h, data):
        h.copy_(self.torch.from_numpy(np.ascontiguousarray(data)))

    def read(self, h):
        return h.cpu().numpy()

    def addr(self, h, off):
        return h.data_ptr() + off

    def sync(self):
        self.torch.cuda.synchronize()
        _lib.check(_lib.load().lrhip_synchronize(), "synchronize")


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("K,M", [(8, 100), (64, 1024), (1024, 1500), (4096, 4096)])
def test_no_write_past_the_count(K, M, R):
    """device calls into a buffer of exactly max_output samples between guard words, all filled with a sentinel bit pattern, input and output
    aligned and one sample past a 16-byte boundary: a call writes its nframes * D outputs (all finite, the host run's bytes), no byte before
    or after them, and does not depend on the bytes around its input; the last workgroup of each call is partial, the third call completes no
    frame and the fourth two.  One output short of capacity, the call is refused before any launch: nothing is
    written and the stage goes on as if the call had not been made."""
    import torch
    rng = np.random.default_rng(17 * K + M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    T = tile_frames(K, R)
    lens = [(2 * T + 1) * K + 3, (T + 2) * K + 1, K - 5, K + 2]
    y = rand_c(rng, sum(lens))
    want, per_call = run_host(make(K, h, R), y, [int(c) for c in np.cumsum(lens)[:-1]])
    assert per_call[2] == 0 and min(per_call[:2]) > 0 and per_call[3] == 2 * D
    edges = np.concatenate([[0], np.cumsum(per_call)])

    def check(c, got):
        assert got.tobytes() == want[edges[c]:edges[c + 1]].tobytes(), c

    mem = TorchMemory()
    for off in (0, 1):
        GD.run_guarded(lambda: make(K, h, R), [y], lens, off, off, mem=mem, call=lambda obj, ins, n, outs, cap: obj.process_device(ins[0], n, outs[0], cap),
                       max_output=lambda obj, n: obj.max_output(n), out_dtype=np.complex64, check=check)

    blk = make(K, h, R)
    sent = int(np.array(GD.SENT).view(np.int32))
    xd = torch.from_numpy(y.view(np.float32).copy()).cuda()
    yd = torch.full((2 * per_call[0] + 64,), sent, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(Exception, match="capacity"):
        blk.process_device(xd.data_ptr(), lens[0], yd.data_ptr(), per_call[0] - 1)
    _lib.load().lrhip_synchronize()
    assert np.all(yd.cpu().numpy().view(np.uint32) == GD.SENT)
    assert blk.process_device(xd.data_ptr(), lens[0], yd.data_ptr(), per_call[0]) == per_call[0]
    _lib.load().lrhip_synchronize()
    out = yd.cpu().numpy()
    assert out[:2 * per_call[0]].view(np.complex64).tobytes() == want[:per_call[0]].tobytes()
    assert np.all(out[2 * per_call[0]:].view(np.uint32) == GD.SENT)


@pytest.mark.parametrize("K,M,R", [(8, 23, 4), (64, 1024, 2), (512, 1000, 4), (4096, 8191, 1)])
def test_reset_equals_fresh_object(K, M, R):
    """lrhip_stage_reset: no partial frame, zero history, class 0.  The run before reset() leaves 7 pending values, a full history and, at
    R > 1, a class other than 0"""
    rng = np.random.default_rng(3 * K + M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    ya, yb = rand_c(rng, 51 * K + 7), rand_c(rng, 30 * K)
    blk = make(K, h, R)
    before, _ = run_host(blk, ya, [7, 20 * K + 1])
    assert len(before) == 51 * D
    blk.reset()
    got, _ = run_host(blk, yb, [K + 3])
    fresh, _ = run_host(make(K, h, R), yb, [K + 3])
    assert got.tobytes() == fresh.tobytes()
    assert np.isfinite(got).all() and np.any(got != 0)


def device_round_trip(K, h, R, x):
    """PolyphaseChannelizerBlock -> PolyphaseSynthesizerBlock with the frames kept on the device; returns (xhat, the frames)"""
    import torch
    ana, syn = make_analysis(K, h, R), make(K, h, R)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    cap_y = ana.max_output(len(x))
    yd = torch.empty(2 * cap_y, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ny = ana.process_device(xd.data_ptr(), len(x), yd.data_ptr(), cap_y)
    cap_x = syn.max_output(ny)
    zd = torch.empty(2 * cap_x, dtype=torch.float32, device="cuda")
    nx = syn.process_device(yd.data_ptr(), ny, zd.data_ptr(), cap_x)
    _lib.load().lrhip_synchronize()
    assert ny % K == 0 and nx == ny // K * (K // R)
    return zd[:2 * nx].cpu().numpy().view(np.complex64), yd[:2 * ny].cpu().numpy().view(np.complex64)


@pytest.mark.parametrize("K,R,beta", [(16, 2, 0.5), (64, 2, 0.5)])
def test_round_trip_on_the_device_rrc(K, R, beta):
    """the root-raised-cosine pair of tests/test_synthesizer_cpu.py on the device: xhat K / R against x delayed by M - 1 within 2e-3 relative"""
    M = 16 * K + 1
    h = np.asarray(filter_utils.fir_root_raised_cosine(M, 1.0, beta, K), np.float32)
    n = 96 * K
    x = rand_c(np.random.default_rng(1000 * K + R), n)
    xhat, _ = device_round_trip(K, h, R, x)
    got, want = xhat.astype(np.complex128)[M - 1:n], x.astype(np.complex128)[:n - (M - 1)]
    resid = float(np.linalg.norm(got * K / R - want) / np.linalg.norm(want))
    print("device rrc round trip K=%d R=%d: residual %.3e" % (K, R, resid))
    assert resid <= 2e-3


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("K", [8, 16])
def test_round_trip_on_the_device_exact_identity(K, R):
    """h = [0, 1, ..., 1] into the analysis bank and g = ones(K) / K out of it: every output within the per-output bar of R x[n - K], the bar
    taken on the frames the device analysis bank produced"""
    import torch
    D = K // R
    n = 37 * K + 3
    x = rand_c(np.random.default_rng(K + R), n)
    ha = np.concatenate([[0.0], np.ones(K)]).astype(np.float32)
    g = np.full(K, 1.0 / K, np.float32)
    ana, syn = make_analysis(K, ha, R), make(K, g, R)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    cap_y = ana.max_output(n)
    yd = torch.empty(2 * cap_y, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ny = ana.process_device(xd.data_ptr(), n, yd.data_ptr(), cap_y)
    cap_x = syn.max_output(ny)
    zd = torch.empty(2 * cap_x, dtype=torch.float32, device="cuda")
    nx = syn.process_device(yd.data_ptr(), ny, zd.data_ptr(), cap_x)
    _lib.load().lrhip_synchronize()
    assert nx == ny // K * D >= n
    xhat = zd[:2 * nx].cpu().numpy().view(np.complex64).astype(np.complex128)
    frames = yd[:2 * ny].cpu().numpy().view(np.complex64)
    _, B = SR.synthesize_f64(frames, g, K, R)
    want = np.concatenate([np.zeros(K), R * x.astype(np.complex128)])[:nx]
    lim = (2 * K * R + 2) * SR.U32 * B[:n]                   # Q = ceil(K / D) = R
    err = xhat[:n] - want[:n]
    assert np.isfinite(xhat).all()
    assert np.all(np.abs(err.real) <= lim) and np.all(np.abs(err.imag) <= lim), float(np.max(np.abs(err) / np.maximum(lim, 1e-300)))


def test_equal_to_the_definition_at_size():
    """K = 64, M = 1024, R = 2, 2^20 input values in one device call (a full grid: interior tiles and the tile remap), every output within the bars"""
    import torch
    K, M, R = 64, 1024, 2
    rng = np.random.default_rng(424242 + K)
    h = O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    n = 1 << 20
    y = rand_c(rng, n)
    blk = make(K, h, R)
    xd = torch.from_numpy(y.view(np.float32)).cuda()
    cap = blk.max_output(n)
    zd = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = blk.process_device(xd.data_ptr(), n, zd.data_ptr(), cap)
    _lib.load().lrhip_synchronize()
    assert got == n // K * (K // R) == cap
    bars(zd[:2 * got].cpu().numpy().view(np.complex64), y, h, K, R, "at size 2^20")
