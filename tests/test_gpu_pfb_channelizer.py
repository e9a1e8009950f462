"""PolyphaseChannelizerBlock with method = "fft" (pfb_channelizer_kernel<F>, kernels_pfb.h) against the float64 filterbank of
tests/helpers/channelizer_ref.py over its accepted domain (K a power of two in [8, 4096], K <= M <= min(64 K, 65536)), against the GEMM block
on the shapes both accept, and the promises that do not depend on rounding: a frame is a pure function of its window, so every chunking and
every entry path gives the same bytes; a frame reads exactly its own window; a call writes exactly its frames.

The bars are the project's bars for this block (tests/test_gpu_channelizer.py): per output and component (2M + 2) 2^-24 B[m], over all outputs
rms(|got - ref| / (2^-24 B[m])) <= 0.3 (2M)^(1/4).  A P-term fmaf sum followed by log2 K butterfly levels is bounded by roughly
(P + 1 + 5 log2 K) 2^-24 B[m], below 2M + 2 for every accepted shape; both are caps, not the expected value."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from oracle import oracle as O
from tests.helpers import channelizer_ref as CR

pytestmark = pytest.mark.gpu


def tile_frames(K):
    """frames per workgroup (PfbChannelizerStage::frames_per_tile)"""
    return 2048 // K if K <= 256 else 8 if K == 512 else 4 if K == 1024 else 8192 // K


def make(K, taps, method="fft"):
    blk = lr.PolyphaseChannelizerBlock(K, taps, {"method": method})
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


def run_host(blk, x, cuts=()):
    """process() over x cut at the given stream positions; returns ([frames, K], frames per call)"""
    parts, a = [], 0
    for b in list(cuts) + [len(x)]:
        parts.append(blk.process(x[a:b]))
        a = b
    return np.concatenate(parts), [len(p) for p in parts]


def agg_bar(M):
    return 0.3 * (2 * M) ** 0.25


class DeviceStream:
    """the whole stream resident on the device, `offset` complex64 samples past a 16-byte boundary; calls are slices of it (process_device)
    and their outputs land back to back"""

    def __init__(self, blk, x, K, offset=0):
        import torch
        self.torch, self.blk, self.K, self.offset = torch, blk, K, offset
        self.xd = torch.from_numpy(np.concatenate([np.zeros(offset, np.complex64), x]).view(np.float32)).cuda()
        F = CR.nframes(len(x), K)
        self.yd = torch.empty(2 * K * (F + 2), dtype=torch.float32, device="cuda")
        self.frames = 0
        torch.cuda.synchronize()

    def call(self, a, b):
        cap = self.yd.numel() // 2 - self.frames * self.K
        got = self.blk.process_device(self.xd.data_ptr() + 8 * (self.offset + a), b - a, self.yd.data_ptr() + 8 * self.K * self.frames, cap)
        _lib.load().lrhip_synchronize()
        assert got % self.K == 0
        self.frames += got // self.K
        return got // self.K

    def result(self):
        self.torch.cuda.synchronize()
        return self.yd[:2 * self.K * self.frames].cpu().numpy().view(np.complex64).reshape(-1, self.K)


def m_values(K):
    return [K, K + 1, 3 * K - 1, 16 * K, min(64 * K, 65536)]


SHAPES = [(K, M) for K in (8, 16, 64, 256, 1024, 4096) for M in sorted(set(m_values(K)))]


def test_the_block_is_the_fft_stage():
    """method = "fft" builds the polyphase + FFT stage (also where the GEMM accepts the shape), no method on a shape the GEMM refuses too"""
    L = _lib.load()
    for blk in (make(64, np.ones(1024, np.float32)), ):
        assert L.lrhip_stage_max_output(blk._stage, 640) == 11 * 64
    blk = lr.PolyphaseChannelizerBlock(256)
    blk.rate = 2.0
    blk.differentiate([types.ComplexFloat32])
    blk.initialize()
    assert len(blk.taps) == 4096
    x = rand_c(np.random.default_rng(1), 256 * 20)
    got = blk.process(x)
    ref, B = CR.channelize_f64(x, blk.taps, 256)
    CR.check_bars(got, ref, B, 4096, agg_bar(4096))
    with pytest.raises(Exception, match="nchannels must be 32 or 64"):
        make(256, np.ones(4096, np.float32), "gemm")


@pytest.mark.parametrize("K,M", SHAPES)
def test_shape_matrix_vs_f64(K, M):
    """3 whole tiles and a partial one (T // 2 + 1 frames) over two calls, the second starting
    inside a hop and reading the history, for a Hamming lowpass and random taps at input scales 1e-3, 1 and 1e3.  Every frame is checked
    (B[m] > 0 for all of them: frame 0 holds x[0])."""
    rng = np.random.default_rng(K * 10007 + M)
    T = tile_frames(K)
    F = 3 * T + T // 2 + 1
    n = (F - 1) * K + 5
    cut = (T + T // 2) * K + 3
    for kind in ("lowpass", "random"):
        h = prototype(kind, M, K, rng)
        for scale in (1e-3, 1.0, 1e3):
            x = rand_c(rng, n, scale)
            ref, B = CR.channelize_f64(x, h, K)
            got, per_call = run_host(make(K, h), x, [cut])
            assert got.shape == (F, K) and sum(per_call) == F and min(per_call) > 0
            r = CR.check_bars(got, ref, B, M, agg_bar(M))
            print("pfb error ratio K=%d M=%d %s scale=%g: rms %.4f max %.4f (bars %.2f, %d)"
                  % (K, M, kind, scale, r, float(np.max(CR.error_ratio(got, ref, B))), agg_bar(M), 2 * M + 2))


@pytest.mark.parametrize("K,M", [(64, 1024), (64, 4096), (32, 96), (32, 1024)])
def test_not_less_accurate_than_the_gemm(K, M):
    """same x and h through both forms: the rms error ratio of the FFT form does not exceed the GEMM's, measured in this test.  No margin:
    a Float32 model of the FFT form (numpy polyphase sums + complex64 ifft) gives 0.11 / 0.06 (lowpass / random) at (64, 1024) where the
    GEMM measures 0.76 / 0.37."""
    rng = np.random.default_rng(31 * K + M)
    n = 300 * K + 5
    for kind in ("lowpass", "random"):
        h = prototype(kind, M, K, rng)
        x = rand_c(rng, n)
        ref, B = CR.channelize_f64(x, h, K)
        fft, _ = run_host(make(K, h, "fft"), x, [77 * K + 3])
        gemm, _ = run_host(make(K, h, "gemm"), x, [77 * K + 3])
        r_fft = CR.check_bars(fft, ref, B, M, agg_bar(M))
        r_gemm = CR.check_bars(gemm, ref, B, M, agg_bar(M))
        print("pfb vs gemm K=%d M=%d %s: rms error ratio fft %.4f gemm %.4f" % (K, M, kind, r_fft, r_gemm))
        assert r_fft <= r_gemm, (kind, r_fft, r_gemm)


@pytest.mark.parametrize("K,M", [(8, 23), (64, 1000), (256, 4097), (1024, 3071), (4096, 65536), (2048, 2049), (512, 32768)])
def test_chunking_is_bit_invariant(K, M):
    """one call and ragged chunkings give identical bytes: calls of 0, 1, K - 1, K, K + 1 samples, calls shorter than M - 1 (the window
    spans the history), calls that produce no frame, and calls of several tiles (interior workgroups take the unchecked load path, the
    first and the last the checked one); host process() pieces, and process_device slices of a resident stream 0 and 1 complex64 samples
    past a 16-byte boundary.  Every tiling class: K <= 256, 512, 1024, 2048, 4096."""
    rng = np.random.default_rng(K + 3 * M)
    h = prototype("random", M, K, rng)
    T = tile_frames(K)
    P = (M + K - 1) // K
    big = (3 * T + P + 2) * K                             # long enough for an interior tile whatever the carried index
    if K * big > 1 << 23:
        big = (T + P + 2) * K
    small = [1, 0, K - 1, K, K + 1, max(1, (M - 1) // 2), 1, K - 1, 3, min(M + 7, 4 * K + 7)]
    lens = small + [big, big + 1, 2 * K + 1, 0, big + 3, 1, 1, K - 1, big // 2, 5 * K + 3]
    n = sum(lens)
    x = rand_c(rng, n)
    whole, _ = run_host(make(K, h), x)
    ref, B = CR.channelize_f64(x, h, K)
    CR.check_bars(whole, ref, B, M, agg_bar(M))

    cuts = [int(c) for c in np.cumsum(lens)[:-1]]
    got, per_call = run_host(make(K, h), x, cuts)
    assert 0 in per_call, per_call
    assert got.tobytes() == whole.tobytes()

    edges = [0] + cuts + [n]
    for offset in (0, 1):
        ds = DeviceStream(make(K, h), x, K, offset)
        zero = sum(ds.call(a, b) == 0 for a, b in zip(edges[:-1], edges[1:]))
        assert zero > 0
        assert ds.result().tobytes() == whole.tobytes(), offset


def test_a_cut_on_every_residue():
    """K = 16, M = 50: the stream cut after 5 K + j samples for every j < K, and into calls of j + 1 samples throughout"""
    K, M = 16, 50
    rng = np.random.default_rng(16050)
    h = prototype("random", M, K, rng)
    n = 40 * K + 9
    x = rand_c(rng, n)
    whole, _ = run_host(make(K, h), x)
    ref, B = CR.channelize_f64(x, h, K)
    CR.check_bars(whole, ref, B, M, agg_bar(M))
    for j in range(K):
        got, _ = run_host(make(K, h), x, [5 * K + j])
        assert got.tobytes() == whole.tobytes(), j
        got, _ = run_host(make(K, h), x, list(range(j + 1, n, j + 1)))
        assert got.tobytes() == whole.tobytes(), j


@pytest.mark.parametrize("K,M", [(64, 1024), (1024, 16384)])
def test_entry_paths_give_equal_bytes(K, M):
    """host vectors in one call of 2^22 + 3K + 5 samples (cut into pieces by the host path), host calls under the piece threshold, device
    pointers in one call, and small ragged host chunks: the same bytes"""
    rng = np.random.default_rng(99 + K + M)
    h = prototype("lowpass", M, K, rng)
    n = (1 << 22) + 3 * K + 5
    x = rand_c(rng, n)
    pieces, _ = run_host(make(K, h), x)
    one_piece, _ = run_host(make(K, h), x, list(range((1 << 20) - 1, n, (1 << 20) - 1)))
    assert one_piece.tobytes() == pieces.tobytes()
    ds = DeviceStream(make(K, h), x, K)
    ds.call(0, n)
    assert ds.result().tobytes() == pieces.tobytes()
    cuts = np.cumsum(rng.integers(1, 40000, n // 20000))
    small, _ = run_host(make(K, h), x, [int(c) for c in cuts if c < n])
    assert small.tobytes() == pieces.tobytes()


def _footprint_positions(n1, n, K, M, T):
    F1 = (n1 + K - 1) // K                             # first frame of call 2
    gl, gf = F1 + T - 1, F1 + T                        # the last frame of call 2's first workgroup and the first of its second
    pos = {"first of call 2": n1, "last of call 1": n1 - 1, "past the last frame": n - 1, "newest sample of the last frame": (n - 1) // K * K,
           "end of workgroup 0": gl * K, "start of workgroup 1": max(0, gf * K - (M - 1)),
           "interior tile": (F1 + 2 * T) * K + K // 2}
    h0 = F1 * K - (M - 1)                              # the oldest sample call 2's first frame takes from the carried history
    if 0 <= h0 < n1:
        pos["history of call 2"] = h0
    return pos


@pytest.mark.parametrize("K,M", [(8, 27), (64, 1000), (64, 65), (256, 700), (1024, 2500), (4096, 9000)])
def test_window_footprint(K, M):
    """a NaN (real part), and separately an Inf (imaginary part), at sample s: exactly the frames {m : mK - (M - 1) <= s <= mK} are
    non-finite in all K channels, every other output is finite.  M is not a multiple of K, so the last tap row is partly padding: a frame
    whose padded row covers s but whose M-sample window does not must stay finite (the kernel skips the padding instead of multiplying by
    zero).  A channel counts as reached when either component is non-finite: with real taps an Inf in Im x leaves Re y_0 = sum h Re x
    finite by definition, and the polyphase form keeps that where the GEMM's 0 * Inf does not."""
    rng = np.random.default_rng(5 * K + M)
    h = prototype("random", M, K, rng)
    T = tile_frames(K)
    P = (M + K - 1) // K
    n1 = (P + 2) * K + 7
    n = n1 + (4 * T + P) * K + 5
    base = rand_c(rng, n)
    F = CR.nframes(n, K)
    m = np.arange(F)
    for name, s in _footprint_positions(n1, n, K, M, T).items():
        for v in (np.nan, np.inf):
            x = base.copy()
            x[s] = complex(v, 0) if np.isnan(v) else complex(0, v)
            got, _ = run_host(make(K, h), x, [n1])
            assert got.shape == (F, K)
            hit = (m * K - (M - 1) <= s) & (s <= m * K)
            assert hit.any() == (name != "past the last frame")     # a sample no frame has reached yet makes nothing non-finite
            nonfin = ~(np.isfinite(got.real) & np.isfinite(got.imag))    # either component not finite
            assert nonfin[hit].all(), (name, s, v, np.flatnonzero(hit)[:3], np.argwhere(~nonfin & hit[:, None])[:4])
            assert not nonfin[~hit].any(), (name, s, v, np.flatnonzero(hit)[:3], np.argwhere(nonfin & ~hit[:, None])[:4])


@pytest.mark.parametrize("K,M", [(8, 100), (64, 1024), (1024, 1500), (4096, 4096)])
@pytest.mark.parametrize("misalign", [0, 1])
def test_no_write_past_the_count(K, M, misalign):
    """device calls into a buffer of exactly max_output samples followed by guard words, all filled with a sentinel bit pattern: the call
    writes its nframes * K outputs (all finite, equal to the host run) and no byte after them; the last workgroup of each call is partial.
    misalign = 1 puts the output 8 bytes past a 16-byte boundary (the kernel's 8-byte store path)."""
    import torch
    rng = np.random.default_rng(17 * K + M)
    h = prototype("random", M, K, rng)
    T = tile_frames(K)
    n1, n2 = 5 * T * K + 3, 2 * T * K + K + 2          # 5 T + 1 frames, then (from K - 3 samples into a hop) 2 T + 1
    x = rand_c(rng, n1 + n2)
    want, _ = run_host(make(K, h), x, [n1])
    blk = make(K, h)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    SENT = np.uint32(0xFFC0DE5A)                         # a NaN payload no kernel computes
    sent_i32 = int(np.array(SENT).view(np.int32))
    done = 0
    for a, b in ((0, n1), (n1, n1 + n2)):
        cap = blk.max_output(b - a)
        yd = torch.full((2 * (misalign + cap + 4096),), sent_i32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got = blk.process_device(xd.data_ptr() + 8 * a, b - a, yd.data_ptr() + 8 * misalign, cap)
        _lib.load().lrhip_synchronize()
        assert got % K == 0 and 0 < got <= cap
        assert (got // K) % T == 1
        y = yd.cpu().numpy().view(np.uint32)
        assert np.all(y[:2 * misalign] == SENT)
        y = y[2 * misalign:]
        assert np.all(y[2 * got:] == SENT), int(np.argmax(y[2 * got:] != SENT)) + 2 * got
        out = y[:2 * got].view(np.float32)
        assert np.isfinite(out).all()
        assert out.view(np.complex64).tobytes() == want[done:done + got // K].tobytes()
        done += got // K
    assert done == len(want)


@pytest.mark.parametrize("K,M", [(64, 1024), (1024, 16384)])
def test_equal_to_the_definition_at_size(K, M):
    """2^24 samples in one call, every one of the 2^24 outputs within the bars of the float64 filterbank"""
    rng = np.random.default_rng(424242 + K)
    h = O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    x = rand_c(rng, 1 << 24)
    got, _ = run_host(make(K, h), x)
    ref, B = CR.channelize_f64(x, h, K)
    r = CR.check_bars(got, ref, B, M, agg_bar(M))
    print("pfb error ratio at size K=%d M=%d 2^24: rms %.4f" % (K, M, r))


@pytest.mark.parametrize("K,M", [(8, 23), (64, 1024), (512, 1000), (4096, 8191)])
def test_reset_equals_fresh_object(K, M):
    """lrhip_stage_reset: zero history and frame phase; the same input afterwards gives the bytes of a new object"""
    rng = np.random.default_rng(3 * K + M)
    h = prototype("random", M, K, rng)
    xa, xb = rand_c(rng, 50 * K + 13), rand_c(rng, 30 * K + 29)
    blk = make(K, h)
    run_host(blk, xa, [7, 20 * K + 1])
    blk.reset()
    got, _ = run_host(blk, xb, [K + 3])
    fresh, _ = run_host(make(K, h), xb, [K + 3])
    assert got.tobytes() == fresh.tobytes()
    assert np.isfinite(got).all() and np.any(got != 0)
