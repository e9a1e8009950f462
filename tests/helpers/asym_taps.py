"""Asymmetric taps for every decimating, interpolating and fused real-tap FIR form: the tap generators, the case table of
tests/test_gpu_asym_taps.py and, for every case, a reference built from oracle/oracle.py stages only.  Importable without a GPU
(tests/test_asym_taps_cpu.py holds the table to its purpose there).

Why: a Hamming-window lowpass is exactly symmetric in Float32, h[k] == h[M-1-k], so a kernel that walks its taps backwards - or a polyphase /
Toeplitz table built mirrored - produces the same terms in the same order and passes even a bit-exact comparison.  With these taps it does not.

Stream lengths: with T the outputs of one tile of the form (tests/test_gpu_bounds.py TILES and the lines it cites, restated by mfma_tile() /
lds_tile() below) a case runs 3 T D + T D / 2 + 7 input samples, once whole and once as calls of 1, 2 T D + 3 and the rest; a case that decimates
also as calls of 1, 1, 2 T D + 3 and the rest, whose second call emits nothing (idle_call_lengths)."""
import collections
import zlib

import numpy as np

from luaradio_amd import filter_utils
from oracle import oracle as O

FS = 1102500.0
GAIN = 1.25
BITS = "bits"          # a bar of BITS is bit equality


# ------------------------------------------------------------------------------------------------------------------------ taps
def random_taps(rng, M):
    """uniform(-1, 1) / M; both end taps at least 0.25 / M in magnitude, so an off-by-one at either end is far above every bar"""
    h = (rng.uniform(-1, 1, M) / M).astype(np.float32)
    for k in sorted({0, M - 1}):
        while abs(h[k]) < 0.25 / M:
            h[k] = np.float32(rng.uniform(-1, 1) / M)
    return h


def skewed_lowpass(M, cutoff):
    """Hamming lowpass times a ramp 0.6 .. 1.4, unit DC gain: as well conditioned in front of a discriminator as the lowpass itself, and not symmetric"""
    h = np.asarray(filter_utils.firwin_lowpass(M, cutoff), np.float64) * np.linspace(0.6, 1.4, M)
    return (h / np.sum(h)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ tiles
def mfma_tile(cplx, D):
    """kernels_fir.h:184 tile_out = nw * nacc * (16 / S) * 16 with the accumulators per wave of stage_fir.h dispatch_mfma"""
    nacc = {1: 8, 2: 4, 3: 2, 4: 2, 5: 2}.get(D, 1)
    return 4 * nacc * (8 if cplx else 16) * 16


def lds_tile(M, D, second_form, disc=0):
    """stage_fir.h launch_decim_lds: OW = (span_max - M) / D + 1 - dsc, at most 256 - 4 dsc; span_max = DECIM2_SPAN_MAX 6128 / DECIM_SPAN_MAX 6144"""
    return min(256 - 4 * disc, ((6128 if second_form else 6144) - M) // D + 1 - disc)


DECFFT_TILE = 3584      # stage_fir.h launch_decfft_d: workgroups of 4 waves x one quad of 4 blocks, kernels_firdecfft.h:55 DF_LO = 224 outputs per block
PAIR_TILE = 2560        # stage_fir.h launch_win_cplx_m: ntiles over 2 * G::TO, TO = 256 * 5
PASS1024R_TILE = 1792   # stage_fir.h launch_fft: Lf = 1024 - 128 = 896, two blocks of a Float32 stream per transform
D1_TILE = 4096          # stage_fir.h dispatch_mfma: launch_mfma<2, 1, 8>


def stream_len(T, D):
    return 3 * T * D + T * D // 2 + 7


def call_lengths(n, T, D):
    """the chunked run of a case: calls of 1, 2 T D + 3 and the rest"""
    a = 2 * T * D + 3
    return [1, a, n - 1 - a]


def idle_call_lengths(n, T, D):
    """a second chunking for D >= 2: calls of 1, 1, 2 T D + 3 and the rest.  The first call leaves the decimation index at D - 1, so the second one
    emits nothing: no filter launch, the history is carried by its own kernel, and no discriminator or recurrence state may move"""
    assert D >= 2
    a = 2 * T * D + 3
    return [1, 1, a, n - 2 - a]


def chunkings(case):
    """the chunked runs of a case: call_lengths, and idle_call_lengths where the case decimates (at D = 1 every call emits)"""
    return [call_lengths(case.n, case.T, case.D)] + ([idle_call_lengths(case.n, case.T, case.D)] if case.D >= 2 else [])


# ------------------------------------------------------------------------------------------------------------------------ cases
# group: the section of the GPU test; form: the kernel form or fused chain the case is there for; stream: "cf32" / "f32"; bar: BITS or the tolerance
# against reference(case); p: the parameters the GPU test builds the blocks from
Case = collections.namedtuple("Case", "group form stream name bar n T D taps p")

# what the table must cover: every (form, stream type) pair
FORMS = [
    ("MfmaPersistent", "cf32"), ("MfmaPersistent", "f32"), ("MfmaGeneric", "cf32"), ("MfmaGeneric", "f32"), ("DecimLds2", "cf32"), ("DecimLds1", "f32"),
    ("DecFft", "cf32"), ("WinPair", "f32"),
    ("tuner", "cf32"), ("disc-epilogue", "cf32"), ("disc-front", "cf32"), ("unary-fold", "cf32"), ("polyphase-tail", "f32"), ("receiver", "cf32"),
    ("interp", "cf32"), ("rational", "cf32"), ("resample", "f32"), ("resample", "cf32"), ("resample-unfused", "f32"), ("resample-unfused", "cf32"),
]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _fir_case(form, cplx, M, D, use_fft=False, T=None, bar=BITS):
    stream = "cf32" if cplx else "f32"
    name = "%s-%s-m%d-d%d" % (form, stream, M, D)
    if T is None:
        T = mfma_tile(cplx, D)
    return Case("fir", form, stream, name, bar, stream_len(T, D), T, D, (random_taps(_rng(name), M),), {"use_fft": use_fft})


def fir_cases():
    """section A: one FIR stage, FIRFilterBlock(taps, use_fft) with .decimation = D.  Each shape is a row "asym: <name>" (or an older row) of
    tools/host_fir_form_check.hip, which pins the form it names"""
    out = [_fir_case("MfmaPersistent", True, 128, 5), _fir_case("MfmaPersistent", False, 126, 5),
           # 124 taps at D = 5 on a Float32 stream are (3 + 75 + 124 + 3) / 4 = 51 steps: the persistent instantiation, not the generic one (122 taps: 50 steps)
           _fir_case("MfmaPersistent", False, 124, 5), _fir_case("MfmaGeneric", False, 122, 5), _fir_case("MfmaGeneric", True, 124, 5)]
    for cplx in (True, False):
        out += [_fir_case("MfmaGeneric", cplx, 128, D) for D in (2, 3, 4, 6, 7, 8, 10)]
        out += [_fir_case("MfmaGeneric", cplx, 33, D) for D in (2, 5)]
    # all four residues of D mod 4, tap counts that are no multiple of 4, a filter shorter than one group of sixteen
    out += [_fir_case("DecimLds2", True, M, D, T=lds_tile(M, D, True)) for D, M in ((9, 33), (12, 40), (18, 77), (75, 128), (50, 13))]
    out += [_fir_case("DecimLds1", False, M, D, T=lds_tile(M, D, False)) for D, M in ((9, 33), (50, 128), (25, 77))]
    # ceil(M / D) <= 32 up to its edge
    out += [_fir_case("DecFft", True, M, D, "fast", DECFFT_TILE, 1e-6) for D, M in ((2, 33), (2, 64), (4, 128), (5, 128), (5, 160), (8, 128), (8, 256))]
    out.append(_fir_case("WinPair", False, 136, 5, T=PAIR_TILE))
    return out


def _hz(cutoff, rate):
    return cutoff / (rate / 2)


def chain_cases():
    """section B: fused chains, FIRFilterBlock(skewed_lowpass) where the existing tests put LowpassFilterBlock"""
    out = []
    # ---- tuner [FrequencyTranslator, FIR, Downsampler(D)]: persistent and generic Toeplitz with the rotator, the second LDS-staged form with it
    for D, T, offset, cutoff in ((5, mfma_tile(True, 5), -250e3, _hz(100e3, FS)), (4, mfma_tile(True, 4), -250e3, _hz(100e3, FS)),
                                 (50, lds_tile(128, 50, True), -100e3, 0.8 / 50), (80, lds_tile(128, 80, True), -100e3, 0.8 / 80)):
        out.append(Case("tuner", "tuner", "cf32", "tuner-d%d" % D, 2e-6, stream_len(T, D), T, D, (skewed_lowpass(128, cutoff),),
                        {"rate": FS, "offset": offset, "toeplitz": D < 9}))
    # ---- discriminator epilogue.  bar: disc_err() against the unfused device blocks, BITS where the existing tests require the bits
    def disc(name, D, T, rate, offset, cutoff, bar, **p):
        p.update(rate=rate, offset=offset)
        return Case("disc", "disc-epilogue", "cf32", name, bar, stream_len(T, D), T, D, (skewed_lowpass(128, cutoff),), p)
    out += [disc("disc-tuner-d5", 5, mfma_tile(True, 5), FS, -250e3, _hz(100e3, FS), 2e-6, max_launches=2),
            disc("disc-tuner-d5-exact", 5, mfma_tile(True, 5), FS, -250e3, _hz(100e3, FS), BITS, max_launches=2, env="LRHIP_TUNER_EXACT"),
            disc("disc-fir-d1", 1, D1_TILE, FS, None, _hz(100e3, FS), BITS, max_launches=2)]
    out += [disc("disc-tuner-d%d" % D, D, mfma_tile(True, D), 220500.0 * D, -250e3, _hz(100e3, 220500.0 * D), 2e-6, max_launches=2) for D in (4, 8, 10)]
    out += [disc("disc-lds2-d50", 50, lds_tile(128, 50, True, 1), FS, -100e3, 0.8 / 50, BITS, launches=1),
            disc("disc-decfft-d5", 5, DECFFT_TILE, FS, -250e3, _hz(100e3, FS), 2e-6, launches=1, use_fft="fast")]
    # ---- discriminator in front (plan_disc_fir): the discriminator runs in the overlap-save kernel's load stage
    T = PASS1024R_TILE
    out.append(Case("disc-front", "disc-front", "cf32", "disc-front", 1e-6, stream_len(T, 1), T, 1, (random_taps(_rng("disc-front"), 128),), {"launches": 2}))
    # ---- complex -> real block folded into the LDS-staged decimator's store
    T = lds_tile(77, 18, True)
    out.append(Case("unary", "unary-fold", "cf32", "unary-fold", BITS, stream_len(T, 18), T, 18, (skewed_lowpass(77, 1 / 18),), {"launches": 1}))
    # ---- polyphase tail [FIR(h, "auto"), FMDeemphasisFilter, Downsampler(D)]: the pair-mode kernel with the recurrence on its accumulators, the low-rate
    # recurrence as its own launch (g has 68 taps: the generic Toeplitz kernel), the widest fold (g has 144 taps at D = 16: the first LDS-staged form)
    # random taps (the bar is the plain 1e-6, no discriminator, no rotator): behind the de-emphasis a reversed skewed lowpass moves the output by 0.011 .. 0.016 only
    for M, D, T, launches in ((128, 5, PAIR_TILE, (1, 1)), (64, 3, mfma_tile(False, 3), (3, 3)), (128, 16, lds_tile(144, 16, False), (1, 4))):
        name = "tail-m%d-d%d" % (M, D)
        out.append(Case("tail", "polyphase-tail", "f32", name, 1e-6, stream_len(T, D), T, D, (random_taps(_rng(name), M),),
                        {"rate": 220500.0, "tau": 75e-6, "launches_range": launches}))
    # ---- the one-launch receiver (kernels_rx.h) and its two-launch form: the shapes RxStage::shapes_ok merges.  The tuner's filter feeds the discriminator:
    # skewed lowpass.  The audio filter does not, and a reversed skewed lowpass behind the de-emphasis moves the audio by less than 0.02: random taps
    for name, launches in (("rx-one-launch", 1), ("rx-two-launch", 2)):
        out.append(Case("rx", "receiver", "cf32", name, (1e-5, 1e-4), 1 << 17, 25600 // 25, 25,
                        (skewed_lowpass(128, _hz(100e3, FS)), random_taps(_rng("rx-audio"), 128)),
                        {"rate": FS, "offset": -250e3, "tau": 75e-6, "launches": launches, "cuts": [1, 2, 1281, 70001, 70002]}))
    return out


RESAMPLE_CUTS = [1, 2, 3, 255, 256, 257]


def _resample_case(form, cplx, L, D, M, tile_in, c, fused=True):
    stream = "cf32" if cplx else "f32"
    name = "%s-%s-l%d-d%d-m%d-c%g" % (form, stream, L, D, M, c)
    return Case("resample", form, stream, name, BITS, 4 * tile_in + 7, tile_in, D, (random_taps(_rng("%s-%d-%d-%d" % (form, L, D, M)), M),),
                {"L": L, "c": c, "fused": fused})


def resample_cases():
    """section C: [MultiplyConstant(c)] -> Upsampler(L) -> FIR -> [Downsampler(D)], one polyphase launch (plan_resample).  c = 1: no MultiplyConstantBlock
    (the mc == nullptr branch).  Four tiles of input plus 7"""
    rows = []
    rows += [("interp", True, L, 1, 128, 1280) for L in (2, 3, 4, 5)]                                  # kernels_interp.h TQ = 256 * 5 inputs per tile
    rows += [("rational", True, L, D, 128, 256 * R) for L, D, R in ((3, 2, 6), (2, 3, 9), (4, 3, 6), (3, 4, 8), (5, 4, 8), (4, 5, 10))]      # stage_resample.h:110
    # fir_resample_kernel: 256 outputs per workgroup = 256 D / L inputs.  (25, 4, 16): fewer taps than phases, J = 1.  (2, 47, 128): the last D fits() accepts
    for cplx in (True, False):
        rows += [("resample", cplx, L, D, M, -(-256 * D // L)) for L, D, M in ((2, 1, 77), (7, 3, 96), (25, 4, 16), (4, 25, 130), (2, 47, 128))]
    rows.append(("resample", False, 3, 2, 128, -(-256 * 2 // 3)))
    out = []
    for form, cplx, L, D, M, tile in rows:
        out += [_resample_case(form, cplx, L, D, M, tile, float(L)), _resample_case(form, cplx, L, D, M, tile, 1.0)]
    # a constant that is neither L nor a power of two: the single Float32 product is visible
    out += [_resample_case("rational", True, 3, 2, 128, 256 * 6, 0.3), _resample_case("resample", False, 7, 3, 96, -(-256 * 3 // 7), 0.3)]
    # (2, 48, 128): the first D fits() refuses - the chain does not fuse and still gives the bits
    out += [_resample_case("resample-unfused", cplx, 2, 48, 128, 256 * 48 // 2, 2.0, fused=False) for cplx in (True, False)]
    return out


def all_cases():
    return fir_cases() + chain_cases() + resample_cases()


# ------------------------------------------------------------------------------------------------------------------------ inputs
def rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


def fm_tone(rng, n, rate, carrier):
    """an FM tone (400 Hz, 2.5 kHz deviation) on the carrier plus 0.05 noise: the input of test_lds_staged_decimator_discriminator_epilogue, carrier at
    the translator's own offset as there - the translator moves it out of the filter's band, so the angles are those of the filtered noise, which reversed
    taps move by a quarter of the rms and more (with the tone in band a reversed near-linear-phase lowpass only delays a 400 Hz message: below 0.02)"""
    t = np.arange(n) / rate
    return (np.exp(2j * np.pi * (carrier * t + 2.5e3 / 400.0 * np.sin(2 * np.pi * 400.0 * t))) + 0.05 * rand_c(rng, n)).astype(np.complex64)


def case_input(case):
    rng = _rng("x-" + case.name.replace("-exact", "").replace("-two-launch", "-one-launch"))
    if case.group in ("disc", "rx"):
        off = case.p["offset"]
        return fm_tone(rng, case.n, case.p["rate"], off if off is not None else -250e3)
    if case.stream == "cf32":
        return rand_c(rng, case.n)
    return rng.uniform(-1, 1, case.n).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ references
def _rotator(case):
    off = case.p.get("offset")
    return [O.Rotator(2 * np.pi * (off / case.p["rate"]), O.MODE_F64)] if off is not None else []


def zero_stuffed(x, L, c):
    """u = zeros(n L), u[::L] = float32(c) * x: one Float32 product per component"""
    u = np.zeros(len(x) * L, x.dtype)
    prod = (np.float32(c) * np.ascontiguousarray(x).view(np.float32)).astype(np.float32)
    u[::L] = prod.view(x.dtype)
    return u


def reference(case, taps=None, mode=None):
    return np.ascontiguousarray(_reference(case, taps, mode))


def _reference(case, taps, mode):
    """the case's reference from oracle stages only.  taps: stand-ins for case.taps (the conditioning check passes them reversed); mode: the recurrence /
    audio arithmetic of the receiver (MODE_LUA by default, as test_wbfm_receiver_launch_forms)"""
    h = tuple(case.taps if taps is None else taps)
    x = case_input(case)
    cplx = case.stream == "cf32"
    D = case.D
    g = case.group
    if g == "fir":
        return O.FIR(h[0], cplx, O.MODE_FMA if case.bar == BITS else O.MODE_F64).process(x)[::D]
    if g == "tuner":
        return O.Chain(_rotator(case) + [O.FIR(h[0], True, O.MODE_FMA)]).process(x)[::D]
    if g == "disc":
        fir_mode = O.MODE_F64 if case.p.get("use_fft") else O.MODE_FMA
        return O.FMDiscriminator(GAIN).process(O.Chain(_rotator(case) + [O.FIR(h[0], True, fir_mode)]).process(x)[::D])
    if g == "disc-front":
        return O.FIR(h[0], False, O.MODE_F64).process(O.FMDiscriminator(GAIN).process(x))
    if g == "unary":
        return np.abs(O.FIR(h[0], True, O.MODE_FMA).process(x)[::D])
    if g == "tail":
        b, a = O.fm_deemphasis_taps(case.p["tau"], case.p["rate"])
        return O.IIR(b, a, False, O.MODE_F64).process(O.FIR(h[0], False, O.MODE_FMA).process(x))[::D]
    if g == "rx":
        mode = O.MODE_LUA if mode is None else mode
        b, a = O.fm_deemphasis_taps(case.p["tau"], case.p["rate"] / 5)
        y = O.Chain(_rotator(case) + [O.FIR(h[0], True, mode), O.Downsampler(5, True), O.FMDiscriminator(GAIN), O.FIR(h[1], False, mode),
                                      O.IIR(b, a, False, mode), O.Downsampler(5, False)]).process(x)
        return y
    if g == "resample":
        return O.FIR(h[0], cplx, O.MODE_FMA).process(zero_stuffed(x, case.p["L"], case.p["c"]))[::D]
    raise ValueError(case.group)


def filter_output(case):
    """the ComplexFloat32 filter outputs in front of the discriminator (what disc_err() weighs a difference with), from the oracle"""
    return O.Chain(_rotator(case) + [O.FIR(case.taps[0], True, O.MODE_FMA)]).process(case_input(case))[::case.D]


def reversed_taps(case, which):
    return tuple(h[::-1].copy() if k == which else h for k, h in enumerate(case.taps))
