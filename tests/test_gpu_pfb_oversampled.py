"""PolyphaseChannelizerBlock with options["oversample"] = R in {2, 4} (pfb_oversampled_kernel<R, F>, kernels_pfb.h: frame hop D = K / R) against
the float64 filterbank of tests/helpers/channelizer_os_ref.py over every tiling class, and the promises that do not depend on rounding: a
frame is a pure function of its window and its class m mod R, so every chunking and every entry path gives the same bytes; frame m R has the
bytes of the critically sampled block's frame m; a frame reads exactly its own window; a call writes exactly its frames; reset() forgets
the class.

The bars are the block's own (tests/test_gpu_pfb_channelizer.py): per output and component (2M + 2) 2^-24 B[m], over all outputs
rms(|got - ref| / (2^-24 B[m])) <= 0.3 (2M)^(1/4).  The rotation moves the polyphase sums before the inverse DFT and adds no arithmetic, so
the bound of a P-term fmaf sum followed by log2 K butterfly levels carries over unchanged."""
import ctypes as C

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from oracle import oracle as O
from tests.helpers import channelizer_os_ref as OS

pytestmark = pytest.mark.gpu


def tile_frames(K, R=4):
    """frames per workgroup of the oversampled kernel (PfbChannelizerStage::launch_oversampled_by_k); only sizes the streams"""
    return 2048 // K if K <= 256 else 2 if K == 4096 else 16 if (K, R) == (512, 4) else 4 if (K, R) == (1024, 2) else 8


def make(K, taps, R):
    options = {"method": "fft"} if R == 1 else {"oversample": R}
    blk = lr.PolyphaseChannelizerBlock(K, taps, options)
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

    def __init__(self, blk, x, K, D, offset=0):
        import torch
        self.torch, self.blk, self.K, self.offset = torch, blk, K, offset
        self.xd = torch.from_numpy(np.concatenate([np.zeros(offset, np.complex64), x]).view(np.float32)).cuda()
        F = OS.nframes(len(x), D)
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


def test_the_block_is_the_oversampled_stage():
    """options["oversample"] builds the stage with hop K / R: max_output(n) = (n / D + 1) K, process() returns [frames, K], get_rate() = R rate"""
    L = _lib.load()
    for R, D in ((2, 32), (4, 16)):
        blk = make(64, np.ones(1024, np.float32), R)
        assert L.lrhip_stage_max_output(blk._stage, 640) == (640 // D + 1) * 64
        assert blk.get_rate() == 2.0 * R
        got = blk.process(rand_c(np.random.default_rng(R), 10 * D + 1))
        assert got.shape == (11, 64)
    with pytest.raises(Exception):
        blk.seek(64)


SHAPES = [(K, M, R) for K in (8, 16, 64, 256, 512, 1024, 2048, 4096) for M in (K, K + 1, 3 * K - 1, 16 * K) for R in (2, 4)]


@pytest.mark.parametrize("K,M,R", SHAPES)
def test_shape_matrix_vs_f64(K, M, R):
    """3 whole tiles and a partial one (T // 2 + 1 frames) over two calls; the first call ends 3 samples into a hop (1 sample at D = 2) after a
    frame count that is not a multiple of R, so the second starts on a class other than 0 and reads the history; a Hamming lowpass and random
    taps at input scales 1e-3, 1 and 1e3.  Every frame is checked (B[m] > 0 for all of them: frame 0 holds x[0])."""
    rng = np.random.default_rng(K * 10007 + M + R)
    D = K // R
    T = tile_frames(K, R)
    n = (3 * T + T // 2) * D + 5
    F = OS.nframes(n, D)
    c1 = T + T // 2
    while OS.nframes(c1 * D + 3, D) % R == 0:
        c1 += 1
    cut = c1 * D + 3
    assert 0 < cut < n
    for kind in ("lowpass", "random"):
        h = prototype(kind, M, K, rng)
        for scale in (1e-3, 1.0, 1e3):
            x = rand_c(rng, n, scale)
            ref, B = OS.channelize_os_f64(x, h, K, R)
            got, per_call = run_host(make(K, h, R), x, [cut])
            assert got.shape == (F, K) and sum(per_call) == F and min(per_call) > 0 and per_call[0] % R != 0
            r = OS.check_bars(got, ref, B, M, agg_bar(M))
            print("oversampled pfb error ratio K=%d M=%d R=%d %s scale=%g: rms %.4f max %.4f (bars %.2f, %d)"
                  % (K, M, R, kind, scale, r, float(np.max(OS.error_ratio(got, ref, B))), agg_bar(M), 2 * M + 2))


@pytest.mark.parametrize("K,M,R", [(8, 23, 4), (64, 1000, 2), (512, 32768, 2), (2048, 2049, 4), (4096, 65536, 2)])
def test_chunking_is_bit_invariant(K, M, R):
    """one call and ragged chunkings give identical bytes: calls of 0, 1, D - 1, D, D + 1 samples, calls shorter than M - 1 (the window
    spans the history), calls that produce no frame, and calls of several tiles (interior workgroups take the unchecked load path, the
    first and the last the checked one); host process() pieces, and process_device slices of a resident stream 0 and 1 complex64 samples
    past a 16-byte boundary."""
    rng = np.random.default_rng(K + 3 * M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    T = tile_frames(K, R)
    P = (M + K - 1) // K
    big = (3 * T + P * R + 2) * D                          # long enough for an interior tile whatever the carried index
    if K * big > 1 << 23:
        big = (T + P * R + 2) * D
    small = [1, 0, D - 1, D, D + 1, max(1, (M - 1) // 2), 1, D - 1, 3, min(M + 7, 4 * D + 7)]
    lens = small + [big, big + 1, 2 * D + 1, 0, big + 3, 1, 1, D - 1, big // 2, 5 * D + 3]
    n = sum(lens)
    x = rand_c(rng, n)
    whole, _ = run_host(make(K, h, R), x)
    ref, B = OS.channelize_os_f64(x, h, K, R)
    OS.check_bars(whole, ref, B, M, agg_bar(M))

    cuts = [int(c) for c in np.cumsum(lens)[:-1]]
    got, per_call = run_host(make(K, h, R), x, cuts)
    assert 0 in per_call, per_call
    assert got.tobytes() == whole.tobytes()

    edges = [0] + cuts + [n]
    for offset in (0, 1):
        ds = DeviceStream(make(K, h, R), x, K, D, offset)
        zero = sum(ds.call(a, b) == 0 for a, b in zip(edges[:-1], edges[1:]))
        assert zero > 0
        assert ds.result().tobytes() == whole.tobytes(), offset


@pytest.mark.parametrize("R", [2, 4])
def test_a_cut_on_every_residue(R):
    """K = 16, M = 50: the stream cut after 5 D + j samples for every j < K (every class and every offset inside a hop at a call's start), and
    into calls of j + 1 samples throughout"""
    K, M = 16, 50
    D = K // R
    rng = np.random.default_rng(16050 + R)
    h = prototype("random", M, K, rng)
    n = 40 * K + 9
    x = rand_c(rng, n)
    whole, _ = run_host(make(K, h, R), x)
    ref, B = OS.channelize_os_f64(x, h, K, R)
    OS.check_bars(whole, ref, B, M, agg_bar(M))
    for j in range(K):
        got, _ = run_host(make(K, h, R), x, [5 * D + j])
        assert got.tobytes() == whole.tobytes(), j
        got, _ = run_host(make(K, h, R), x, list(range(j + 1, n, j + 1)))
        assert got.tobytes() == whole.tobytes(), j


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("K,M", [(64, 1024), (1024, 3071), (4096, 8191)])
def test_frames_m_r_are_the_critically_sampled_frames(K, M, R):
    """frame m R has the window of the {"method": "fft"} block's frame m, rotation 0 and the same accumulation order: the same bytes, over
    several tiles and a cut inside a hop"""
    rng = np.random.default_rng(K + M + R)
    h = prototype("random", M, K, rng)
    T = tile_frames(K, R)
    n = (3 * T + T // 2) * K + 5
    cut = (T + 1) * K + 3
    x = rand_c(rng, n)
    crit, _ = run_host(make(K, h, 1), x, [cut])
    got, _ = run_host(make(K, h, R), x, [cut])
    assert len(got) == OS.nframes(n, K // R) and len(got[::R]) == len(crit)
    assert got[::R].tobytes() == crit.tobytes()
    assert np.isfinite(got).all() and np.any(got[1::R] != 0)


@pytest.mark.parametrize("K,M", [(8, 23), (64, 1024), (4096, 8191)])
def test_oversample_one_is_the_critically_sampled_stage(K, M):
    """lrhip_pfb_oversampled_create(..., 1) against lrhip_pfb_channelizer_create: the same stage, the same bytes and the same capacity"""
    L = _lib.load()
    rng = np.random.default_rng(K + M)
    h = prototype("random", M, K, rng)
    x = rand_c(rng, (3 * tile_frames(K) + 1) * K + 5)
    cut = K + 3
    want, _ = run_host(make(K, h, 1), x, [cut])
    blk = make(K, h, 1)
    blk._set_stage(L.lrhip_pfb_oversampled_create(h.ctypes.data_as(C.POINTER(C.c_float)), M, K, 1), "Creating the stage through the new entry point")
    assert blk.max_output(10 * K + 1) == 11 * K
    got, _ = run_host(blk, x, [cut])
    assert got.tobytes() == want.tobytes()


def _footprint_positions(n1, n, D, M, T):
    F1 = (n1 + D - 1) // D                             # first frame of call 2
    gl, gf = F1 + T - 1, F1 + T                        # the last frame of call 2's first workgroup and the first of its second
    pos = {"first of call 2": n1, "last of call 1": n1 - 1, "past the last frame": n - 1, "newest sample of the last frame": (n - 1) // D * D,
           "end of workgroup 0": gl * D, "start of workgroup 1": max(0, gf * D - (M - 1)),
           "interior tile": (F1 + 2 * T) * D + D // 2}
    h0 = F1 * D - (M - 1)                              # the oldest sample call 2's first frame takes from the carried history
    if 0 <= h0 < n1:
        pos["history of call 2"] = h0
    return pos


@pytest.mark.parametrize("K,M,R", [(8, 27, 4), (64, 1000, 2), (1024, 2500, 2), (4096, 9000, 4)])
def test_window_footprint(K, M, R):
    """a NaN (real part), and separately an Inf (imaginary part), at sample s: exactly the frames {m : mD - (M - 1) <= s <= mD} are
    non-finite in all K channels, every other output is finite.  M is not a multiple of K, so the last tap row is partly padding: a frame
    whose padded row covers s but whose M-sample window does not must stay finite.  A channel counts as reached when either component is
    non-finite (with real taps an Inf in Im x leaves Re y_0 finite by definition).  The first call emits a frame count that is not a multiple
    of R."""
    rng = np.random.default_rng(5 * K + M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    T = tile_frames(K, R)
    P = (M + K - 1) // K
    n1 = (P * R + 2) * D + 7
    n = n1 + (4 * T + P * R) * D + 5
    assert OS.nframes(n1, D) % R != 0 and (n - 1) % D != 0
    base = rand_c(rng, n)
    F = OS.nframes(n, D)
    m = np.arange(F)
    for name, s in _footprint_positions(n1, n, D, M, T).items():
        for v in (np.nan, np.inf):
            x = base.copy()
            x[s] = complex(v, 0) if np.isnan(v) else complex(0, v)
            got, _ = run_host(make(K, h, R), x, [n1])
            assert got.shape == (F, K)
            hit = (m * D - (M - 1) <= s) & (s <= m * D)
            assert hit.any() == (name != "past the last frame")     # a sample no frame has reached yet makes nothing non-finite
            nonfin = ~(np.isfinite(got.real) & np.isfinite(got.imag))    # either component not finite
            assert nonfin[hit].all(), (name, s, v, np.flatnonzero(hit)[:3], np.argwhere(~nonfin & hit[:, None])[:4])
            assert not nonfin[~hit].any(), (name, s, v, np.flatnonzero(hit)[:3], np.argwhere(nonfin & ~hit[:, None])[:4])


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("K,M", [(8, 100), (64, 1024), (1024, 1500), (4096, 4096)])
@pytest.mark.parametrize("misalign", [0, 1])
def test_no_write_past_the_count(K, M, R, misalign):
    """device calls into a buffer of exactly max_output samples followed by guard words, all filled with a sentinel bit pattern: the call
    writes its nframes * K outputs (all finite, equal to the host run) and no byte after them; the last workgroup of each call is partial.
    misalign = 1 puts the output 8 bytes past a 16-byte boundary (the kernel's 8-byte store path)."""
    import torch
    rng = np.random.default_rng(17 * K + M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    T = tile_frames(K, R)
    n1, n2 = 5 * T * D + 3, 2 * T * D + D + 2
    x = rand_c(rng, n1 + n2)
    want, _ = run_host(make(K, h, R), x, [n1])
    blk = make(K, h, R)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    SENT = np.uint32(0xFFC0DE5A)                         # a NaN payload no kernel computes
    sent_i32 = int(np.array(SENT).view(np.int32))
    done = 0
    for a, b in ((0, n1), (n1, n1 + n2)):
        cap = blk.max_output(b - a)
        assert cap == ((b - a) // D + 1) * K
        yd = torch.full((2 * (misalign + cap + 4096),), sent_i32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got = blk.process_device(xd.data_ptr() + 8 * a, b - a, yd.data_ptr() + 8 * misalign, cap)
        _lib.load().lrhip_synchronize()
        assert got % K == 0 and 0 < got <= cap
        assert (got // K) % T != 0
        y = yd.cpu().numpy().view(np.uint32)
        assert np.all(y[:2 * misalign] == SENT)
        y = y[2 * misalign:]
        assert np.all(y[2 * got:] == SENT), int(np.argmax(y[2 * got:] != SENT)) + 2 * got
        out = y[:2 * got].view(np.float32)
        assert np.isfinite(out).all()
        assert out.view(np.complex64).tobytes() == want[done:done + got // K].tobytes()
        done += got // K
    assert done == len(want)


@pytest.mark.parametrize("K,M,R", [(8, 23, 4), (64, 1024, 2), (512, 1000, 4), (4096, 8191, 2)])
def test_reset_equals_fresh_object(K, M, R):
    """lrhip_stage_reset: zero history, index and class.  The run before reset() emits 51 frames, not a multiple of R, so a class that
    survived the reset would rotate every later frame"""
    rng = np.random.default_rng(3 * K + M + R)
    h = prototype("random", M, K, rng)
    D = K // R
    xa, xb = rand_c(rng, 50 * D + 1), rand_c(rng, 30 * K + 29)
    blk = make(K, h, R)
    before, _ = run_host(blk, xa, [7, 20 * D + 1])
    assert len(before) == 51
    blk.reset()
    got, _ = run_host(blk, xb, [K + 3])
    fresh, _ = run_host(make(K, h, R), xb, [K + 3])
    assert got.tobytes() == fresh.tobytes()
    assert np.isfinite(got).all() and np.any(got != 0)


def test_equal_to_the_definition_at_size():
    """K = 64, M = 1024, R = 2, 2^22 samples in one device call (a full grid: interior tiles and the tile remap), every one of the 2^23 outputs
    within the bars of the float64 filterbank"""
    import torch
    K, M, R = 64, 1024, 2
    rng = np.random.default_rng(424242 + K)
    h = O.firwin_lowpass(M, 1.0 / K).astype(np.float32)
    n = 1 << 22
    x = rand_c(rng, n)
    blk = make(K, h, R)
    xd = torch.from_numpy(x.view(np.float32)).cuda()
    cap = blk.max_output(n)
    yd = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = blk.process_device(xd.data_ptr(), n, yd.data_ptr(), cap)
    _lib.load().lrhip_synchronize()
    assert got == (n // (K // R)) * K
    y = yd[:2 * got].cpu().numpy().view(np.complex64).reshape(-1, K)
    ref, B = OS.channelize_os_f64(x, h, K, R)
    r = OS.check_bars(y, ref, B, M, agg_bar(M))
    print("oversampled pfb error ratio at size K=%d M=%d R=%d 2^22: rms %.4f" % (K, M, R, r))
