"""PolyphaseChannelizerBlock (channelizer_kernel<NCT>, kernels_channelizer.h) against the float64 filterbank of tests/helpers/channelizer_ref.py
over the whole accepted domain (K in {32, 64}, M a multiple of 32 up to 8192), and the promises that do not depend on rounding: a frame is a pure
function of its window, so every chunking and every entry path gives the same bytes; a frame reads exactly its own window; a call writes exactly
its frames."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from oracle import oracle as O
from tests.helpers import channelizer_ref as CR

pytestmark = pytest.mark.gpu

MT = 64                   # frames per workgroup (CHAN_MT)


def make(K, taps):
    blk = lr.PolyphaseChannelizerBlock(K, taps)
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


def interior_tiles(M, K, first, n):
    """workgroups of one call whose staged span [xlo, xlo + nsamp) lies inside the call: the only ones that may take the float4 path"""
    F = (n - first + K - 1) // K if n > first else 0
    nsamp = (MT - 1) * K + M
    return [t for t in range((F + MT - 1) // MT) if first + t * MT * K - (M - 1) >= 0 and first + t * MT * K - (M - 1) + nsamp <= n]


def staging_path(first, offset):
    """staging path of an interior workgroup: x + 2 xlo must be 16-byte aligned, xlo = first + f0 K - (M - 1) with K even and M - 1 odd, so
    the path is set by the parity of (offset of x in complex64 samples from a 16-byte boundary + the call's carried first-frame index)"""
    return "float4" if (offset + first) % 2 == 1 else "fallback"


class DeviceStream:
    """the whole stream resident on the device, `offset` complex64 samples past a 16-byte boundary; calls are slices of it (process_device)
    and their outputs land back to back.  Within one contiguous stream (slice start + carried first-frame index) is a multiple of K, so
    every interior workgroup of every call takes the path staging_path(0, offset)."""

    def __init__(self, blk, x, K, offset=0):
        import torch
        self.torch, self.blk, self.K, self.offset = torch, blk, K, offset
        self.xd = torch.from_numpy(np.concatenate([np.zeros(offset, np.complex64), x]).view(np.float32)).cuda()
        F = CR.nframes(len(x), K)
        self.yd = torch.empty(2 * K * (F + 2), dtype=torch.float32, device="cuda")
        self.frames = 0
        self.first = 0                       # stream position of the next frame inside the next call (the stage's carried index)
        self.paths = set()                   # staging paths taken by interior workgroups
        torch.cuda.synchronize()

    def call(self, a, b):
        n, M = b - a, len(self.blk.taps)
        if interior_tiles(M, self.K, self.first, n):
            self.paths.add(staging_path(self.first, self.offset + a))
        cap = self.yd.numel() // 2 - self.frames * self.K
        got = self.blk.process_device(self.xd.data_ptr() + 8 * (self.offset + a), n, self.yd.data_ptr() + 8 * self.K * self.frames, cap)
        _lib.load().lrhip_synchronize()
        assert got % self.K == 0
        f = got // self.K
        self.first = self.first + f * self.K - n
        assert 0 <= self.first < self.K
        self.frames += f
        return f

    def result(self):
        self.torch.cuda.synchronize()
        return self.yd[:2 * self.K * self.frames].cpu().numpy().view(np.complex64).reshape(-1, self.K)


SHAPES = [(K, M) for K in (32, 64) for M in (32, 64, 96, 1024, 1056, 4096, 8192)]


def agg_bar(M):
    """bar on rms(|got - ref| / (2^-24 B[m])), from what the kernel measures on test_shape_matrix_vs_f64's inputs (fixed seeds; the same at
    input scales 1e-3, 1 and 1e3).  Random taps: 0.37-0.40 at every M, the rounding of a sum whose partial sums random-walk, relative to its l1
    weight.  Hamming lowpass, whose large middle taps add coherently: 0.39 (M = 32), 0.42-0.47 (64, 96), 0.76-0.90 (1024, 1056), 1.15-1.39
    (4096), 1.44-1.76 (8192), i.e. 0.10-0.16 (2M)^(1/4).  The bar is 0.3 (2M)^(1/4), at least 1.9x every measured value and 19-76x below the
    2 sqrt(2M) a sum of 2M independent roundings would allow."""
    return 0.3 * (2 * M) ** 0.25


@pytest.mark.parametrize("K,M", SHAPES)
def test_shape_matrix_vs_f64(K, M):
    """41 workgroups, the last one partial (37 of 64 frames), over two calls (the second starts inside a hop and reads the history), for a
    Hamming lowpass and random taps, at input scales 1e-3, 1 and 1e3.  Per output and component |got - ref| <= (2M + 2) 2^-24 B[m]; over all
    outputs rms(|got - ref| / (2^-24 B[m])) <= agg_bar(M).  Measured maxima of the per-output ratio: 2.3-4.6 for M <= 96 and for random
    taps, up to 16.4 for the M = 8192 lowpass (bar 2M + 2)."""
    rng = np.random.default_rng(K * 10007 + M)
    F = 40 * MT + 37
    n = (F - 1) * K + 5
    cut = 17 * MT * K + 3
    for kind in ("lowpass", "random"):
        h = prototype(kind, M, K, rng)
        for scale in (1e-3, 1.0, 1e3):
            x = rand_c(rng, n, scale)
            ref, B = CR.channelize_f64(x, h, K)
            got, per_call = run_host(make(K, h), x, [cut])
            assert got.shape == (F, K) and sum(per_call) == F
            r = CR.check_bars(got, ref, B, M, agg_bar(M))
            print("channelizer error ratio K=%d M=%d %s scale=%g: rms %.4f max %.4f"
                  % (K, M, kind, scale, r, float(np.max(CR.error_ratio(got, ref, B)))))


@pytest.mark.parametrize("K,M", [(64, 1024), (32, 96), (64, 32), (32, 8192), (64, 4096), (32, 1056)])
def test_chunking_is_bit_invariant(K, M):
    """one call and ragged chunkings give identical bytes: calls of 1, K-1, K, K+1 samples, calls shorter than M - 1 (the window spans the
    history), calls that produce no frame, and long calls at even and odd complex64 offsets so that interior workgroups take both staging paths"""
    rng = np.random.default_rng(K + 3 * M)
    h = prototype("random", M, K, rng)
    big = 3 * MT * K + M + 5 * K                      # long enough for an interior workgroup whatever the carried index
    small = [1, K - 1, K, K + 1, max(1, (M - 1) // 2), 1, K - 1, 3, M + 7]
    lens = small + [big, big + 1, 2 * K + 1, big + 3, 1, 1, big + 2, K - 1, big, 5 * K + 3]
    n = sum(lens)
    x = rand_c(rng, n)
    whole, _ = run_host(make(K, h), x)
    ref, B = CR.channelize_f64(x, h, K)
    CR.check_bars(whole, ref, B, M, agg_bar(M))

    cuts = [int(c) for c in np.cumsum(lens)[:-1]]
    got, per_call = run_host(make(K, h), x, cuts)
    assert 0 in per_call, per_call
    assert got.tobytes() == whole.tobytes()
    # the host path stages each call at a 16-byte boundary: the carried index alone picks the path, and these cuts give both
    paths, first = set(), 0
    for L, f in zip(lens, per_call):
        if interior_tiles(M, K, first, L):
            paths.add(staging_path(first, 0))
        first += f * K - L
    assert paths == {"float4", "fallback"}, paths

    # device slices of the stream 0 and 1 samples past a 16-byte boundary: every interior workgroup on one path, then on the other
    edges = [0] + cuts + [n]
    for offset, path in ((0, "fallback"), (1, "float4")):
        ds = DeviceStream(make(K, h), x, K, offset)
        zero = sum(ds.call(a, b) == 0 for a, b in zip(edges[:-1], edges[1:]))
        assert zero > 0
        assert ds.paths == {path}, ds.paths
        assert ds.result().tobytes() == whole.tobytes(), offset


@pytest.mark.parametrize("K,M", [(64, 1024), (32, 96)])
def test_entry_paths_give_equal_bytes(K, M):
    """host vectors in one call of 2^22 + 3K + 5 samples (cut into pieces by the host path), host calls under the piece threshold, device
    pointers in one call, and small ragged host chunks: the same bytes, and within the bars of the float64 filterbank"""
    rng = np.random.default_rng(99 + K + M)
    h = prototype("lowpass", M, K, rng)
    n = (1 << 22) + 3 * K + 5
    x = rand_c(rng, n)
    pieces, _ = run_host(make(K, h), x)
    ref, B = CR.channelize_f64(x, h, K)
    CR.check_bars(pieces, ref, B, M, agg_bar(M))
    one_piece, _ = run_host(make(K, h), x, list(range((1 << 20) - 1, n, (1 << 20) - 1)))
    assert one_piece.tobytes() == pieces.tobytes()
    ds = DeviceStream(make(K, h), x, K)
    ds.call(0, n)
    assert ds.result().tobytes() == pieces.tobytes()
    cuts = np.cumsum(rng.integers(1, 40000, n // 20000))
    small, _ = run_host(make(K, h), x, [int(c) for c in cuts if c < n])
    assert small.tobytes() == pieces.tobytes()


def _footprint_positions(n1, n, K, M):
    F1 = (n1 + K - 1) // K                             # first frame of call 2
    g63, g64 = F1 + MT - 1, F1 + MT                    # the last frame of call 2's first workgroup and the first of its second
    pos = {"first of call 2": n1, "last of call 1": n1 - 1, "last of call 2": n - 1,
           "end of workgroup 0": g63 * K, "start of workgroup 1": max(0, g64 * K - (M - 1))}
    h0 = F1 * K - (M - 1)                              # the oldest sample call 2's first frame takes from the carried history
    if 0 <= h0 < n1:
        pos["history of call 2"] = h0
    return pos


@pytest.mark.parametrize("K,M", [(64, 1024), (32, 96), (64, 32), (64, 64), (32, 8192)])
@pytest.mark.parametrize("odd", [0, 1])
def test_window_footprint(K, M, odd):
    """a NaN, and separately an Inf, at sample s: exactly the frames {m : mK - (M - 1) <= s <= mK} are non-finite in all K channels and both
    components, every other output is finite.  Positions: first / last sample of a call, the history the next call reads, frames 63 / 64 of a
    call (a workgroup boundary; the sample straddles it when M > K).  Call 1 ends 7 or 8 samples into a hop, so call 2's interior workgroups
    take each staging path in one of the two runs."""
    rng = np.random.default_rng(5 * K + M + odd)
    h = prototype("random", M, K, rng)
    n1 = 100 * K + 7 + odd
    n = n1 + 300 * K + 3 * M + 5
    assert interior_tiles(M, K, (n1 + K - 1) // K * K - n1, n - n1)
    base = rand_c(rng, n)
    F = CR.nframes(n, K)
    m = np.arange(F)
    for name, s in _footprint_positions(n1, n, K, M).items():
        for v in (np.nan, np.inf):
            x = base.copy()
            x[s] = complex(v, 0) if np.isnan(v) else complex(0, v)
            got, _ = run_host(make(K, h), x, [n1])
            assert got.shape == (F, K)
            hit = (m * K - (M - 1) <= s) & (s <= m * K)
            fin = np.isfinite(got.real) | np.isfinite(got.imag)          # either component finite
            nonfin = ~(np.isfinite(got.real) & np.isfinite(got.imag))    # either component not
            assert not fin[hit].any(), (name, s, v, np.flatnonzero(hit)[:3], np.argwhere(fin & hit[:, None])[:4])
            assert not nonfin[~hit].any(), (name, s, v, np.flatnonzero(hit)[:3], np.argwhere(nonfin & ~hit[:, None])[:4])


@pytest.mark.parametrize("K,M", [(64, 1024), (32, 8192), (64, 32)])
def test_no_write_past_the_count(K, M):
    """device calls into a buffer larger than max_output, filled with a sentinel bit pattern: the call writes its nframes * K outputs (all
    finite, equal to the host run) and no byte after them; the last workgroup of each call is partial"""
    import torch
    rng = np.random.default_rng(17 * K + M)
    h = prototype("random", M, K, rng)
    n1, n2 = 70 * MT * K + 5 * K + 3, 9 * MT * K + 11 * K + 6
    x = rand_c(rng, n1 + n2)
    want, _ = run_host(make(K, h), x, [n1])
    blk = make(K, h)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    SENT = np.uint32(0xFFC0DE5A)                         # a NaN payload no kernel computes
    sent_i32 = int(np.array(SENT).view(np.int32))
    done = 0
    for a, b in ((0, n1), (n1, n1 + n2)):
        cap = blk.max_output(b - a)
        yd = torch.full((2 * (cap + 4096),), sent_i32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got = blk.process_device(xd.data_ptr() + 8 * a, b - a, yd.data_ptr(), cap)
        _lib.load().lrhip_synchronize()
        assert got % K == 0 and got <= cap and (got // K) % MT != 0
        y = yd.cpu().numpy().view(np.uint32)
        assert np.all(y[2 * got:] == SENT), int(np.argmax(y[2 * got:] != SENT)) + 2 * got
        out = y[:2 * got].view(np.float32)
        assert np.isfinite(out).all()
        assert out.view(np.complex64).tobytes() == want[done:done + got // K].tobytes()
        done += got // K
    assert done == len(want)


def test_headline_size_every_output():
    """BASELINE.json configs[4] at the bench's size: K = 64, M = 1024, 2^24 samples in one call; every one of the 2^24 outputs within the bars"""
    K, M = 64, 1024
    rng = np.random.default_rng(424242)
    h = O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    x = rand_c(rng, 1 << 24)
    got, _ = run_host(make(K, h), x)
    ref, B = CR.channelize_f64(x, h, K)
    r = CR.check_bars(got, ref, B, M, agg_bar(M))
    print("channelizer error ratio headline K=64 M=1024 2^24: rms %.4f" % r)


@pytest.mark.parametrize("K,M", [(64, 1024), (32, 96)])
def test_reset_equals_fresh_object(K, M):
    """lrhip_stage_reset: zero history and frame phase; the same input afterwards gives the bytes of a new object"""
    rng = np.random.default_rng(3 * K + M)
    h = prototype("random", M, K, rng)
    xa, xb = rand_c(rng, 50 * K + 13), rand_c(rng, 200 * K + 29)
    blk = make(K, h)
    run_host(blk, xa, [7, 20 * K + 1])
    blk.reset()
    got, _ = run_host(blk, xb, [K + 3])
    fresh, _ = run_host(make(K, h), xb, [K + 3])
    assert got.tobytes() == fresh.tobytes()
    assert np.isfinite(got).all() and np.any(got != 0)
