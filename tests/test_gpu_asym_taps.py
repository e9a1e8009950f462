"""Every decimating, interpolating and fused real-tap FIR form with taps that are NOT symmetric (tests/helpers/asym_taps.py: the case table, the taps, the
references from oracle stages; tests/test_asym_taps_cpu.py holds the table to its purpose).  A Hamming lowpass is h[k] == h[M-1-k] to the bit, so a kernel
that walks its taps backwards or a mirrored polyphase / Toeplitz table passes every test that uses one; with these taps it is off by 2 % of the output and more.

Each case is three tiles and a half plus 7 samples, run whole and as calls of 1, 2 T D + 3 and the rest (the FIR stage, tuner, discriminator-epilogue and
polyphase-tail rows that decimate also as calls of 1, 1, 2 T D + 3 and the rest: the second call emits nothing), at the bar of the existing test of the same form,
with that test's launch count (or, for one FIR stage, the row "asym: ..." of tools/host_fir_form_check.hip that pins the FirForm of the shape)."""
import os

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from oracle import oracle as O
from tests import golden_util as G
from tests.helpers import asym_taps as A
from tests.test_gpu_parity import disc_err

pytestmark = pytest.mark.gpu

_worst = {}


def _note(group, name, err, bar):
    """the worst err / bar of a group, printed as it grows (pytest -s)"""
    r = err / bar
    if r > _worst.get(group, (-1.0, None))[0]:
        _worst[group] = (r, name)
    print("%s: %s err %.3g / bar %.3g = %.3g (worst of the group so far: %.3g, %s)" % (group, name, err, bar, r, _worst[group][0], _worst[group][1]))


def make(cls, args, in_type, rate, **attrs):
    blk = cls(*args)
    blk.rate = rate
    for k, v in attrs.items():
        setattr(blk, k, v)
    blk.differentiate([in_type])
    blk.initialize()
    return blk


def build(specs, in_type, rate):
    """[(class, args[, attrs])] -> initialized blocks, rate and type propagated down the run"""
    out = []
    for spec in specs:
        b = make(spec[0], spec[1], in_type, rate, **(spec[2] if len(spec) > 2 else {}))
        out.append(b)
        rate, in_type = b.get_rate(), b.get_output_type()
    return out


def tp(case):
    return types.ComplexFloat32 if case.stream == "cf32" else types.Float32


def in_calls(obj, x, lengths):
    parts, a = [], 0
    for m in lengths:
        parts.append(obj.process(x[a:a + m]))
        a += m
    assert a == len(x)
    return np.concatenate(parts)


def chunked_runs(obj, x, case):
    """the case's chunked runs (A.chunkings: calls of 1, 2 T D + 3 and the rest; where it decimates also 1, 1, 2 T D + 3 and the rest, whose second
    call emits nothing), each from a reset state"""
    out = []
    for calls in A.chunkings(case):
        obj.reset()
        out.append(in_calls(obj, x, calls))
    return out


def at_cuts(obj, x, cuts):
    ends = list(cuts) + [len(x)]
    return in_calls(obj, x, [b - a for a, b in zip([0] + ends[:-1], ends)])


def one_by_one(blocks, x):
    """the blocks run one after the other; returns the output and the last block's input"""
    o = x
    for b in blocks:
        o, x = x, b.process(x)
    return x, o


_refs = {}


def ref(case):
    """a case's reference, computed once and shared (read-only)"""
    key = case.name.replace("-exact", "").replace("-two-launch", "-one-launch")
    if key not in _refs:
        r = A.reference(case)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def _ids(cases):
    return [c.name for c in cases]


# ===================================================================================================== A. one FIR stage
@pytest.mark.parametrize("case", A.fir_cases(), ids=_ids(A.fir_cases()))
def test_fir_stage(case):
    """FIRFilterBlock(taps, use_fft) with .decimation = D, the route of test_gpu_bounds.test_fir_form.  Direct forms: the bits of O.FIR(MODE_FMA)[::D];
    the polyphase-FFT decimator: 1e-6 against MODE_F64 and chunked against whole to 5e-7 (test_decimator_polyphase_fft_vs_f64_oracle)"""
    x, want = A.case_input(case), ref(case)
    blk = make(lr.FIRFilterBlock, [case.taps[0], case.p["use_fft"]], tp(case), 2.0, decimation=case.D)
    whole = blk.process(x)
    for got in chunked_runs(blk, x, case):
        assert len(whole) == len(got) == len(want) == (case.n + case.D - 1) // case.D
        if case.bar == A.BITS:
            assert np.array_equal(whole, want), float(np.max(np.abs(whole - want)))
            assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
        else:
            e1, e2, e3 = G.max_abs_err(whole, want), G.max_abs_err(got, want), G.max_abs_err(got, whole)
            _note("DecFft against f64", case.name, max(e1, e2), case.bar)
            _note("DecFft chunked against whole", case.name, e3, 5e-7)
            assert e1 < case.bar and e2 < case.bar and e3 < 5e-7


# ===================================================================================================== B. fused chains
def _tuner_specs(case, with_disc=False):
    p = case.p
    specs = [(lr.FrequencyTranslatorBlock, [p["offset"]])] if p.get("offset") is not None else []
    specs.append((lr.FIRFilterBlock, [case.taps[0], p.get("use_fft", False)]))
    if case.D > 1:
        specs.append((lr.DownsamplerBlock, [case.D]))
    if with_disc:
        specs.append((lr.FrequencyDiscriminatorBlock, [A.GAIN]))
    return specs


TUNERS = [c for c in A.chain_cases() if c.group == "tuner"]


@pytest.mark.parametrize("case", TUNERS, ids=_ids(TUNERS))
def test_tuner(case):
    """[FrequencyTranslator, FIR, Downsampler(D)].  Toeplitz forms (persistent at D = 5, generic at D = 4, both rotating): the bits of the three device
    blocks run one after the other (test_tuner_fused_rotator_fir_downsampler).  Every shape: 2e-6 of O.Rotator(F64) -> O.FIR(FMA)[::D].  The second
    LDS-staged form with the rotator (tap split over the half-waves): the bits of another chunking (test_lds_staged_decimator_second_form_many_tiles)"""
    x, want = A.case_input(case), ref(case)
    rate = case.p["rate"]
    chain = lr.Chain(build(_tuner_specs(case), types.ComplexFloat32, rate))
    whole = chain.process(x)
    assert chain.last_launches <= 2          # one fused kernel + history carry
    apart = one_by_one(build(_tuner_specs(case), types.ComplexFloat32, rate), x)[0] if case.p["toeplitz"] else None
    for got in chunked_runs(chain, x, case):
        assert len(got) == len(whole) == len(want)
        assert np.array_equal(got, whole)
        if case.p["toeplitz"]:
            assert np.array_equal(got, apart)
        err = G.max_abs_err(got, want)
        _note("tuner against the oracle", case.name, err, case.bar)
        assert err < case.bar


DISCS = [c for c in A.chain_cases() if c.group == "disc"]


@pytest.mark.parametrize("case", DISCS, ids=_ids(DISCS))
def test_discriminator_epilogue(case, monkeypatch):
    """[rotator] -> FIR -> [downsampler] -> discriminator as the epilogue of the filter kernel: disc_err() < 2e-6 against the unfused device blocks, the
    bits where the existing tests require them (LRHIP_TUNER_EXACT, the D = 1 filter, the LDS form against tuner chain + discriminator block)"""
    p = case.p
    if p.get("env"):
        monkeypatch.setenv(p["env"], "1")
    x = A.case_input(case)
    rate = p["rate"]
    chain = lr.Chain(build(_tuner_specs(case, True), types.ComplexFloat32, rate))
    whole = chain.process(x)
    if "launches" in p:
        # (A/B knobs of the LDS form, as in test_lds_staged_decimator_discriminator_epilogue: the epilogue off / the first decimator form)
        if case.name != "disc-lds2-d50" or not (os.environ.get("LRHIP_NO_DISC_EPI_LDS") or os.environ.get("LRHIP_DECIM_V1")):
            assert chain.last_launches == p["launches"]
    else:
        assert chain.last_launches <= p["max_launches"]              # fused kernel + wave-boundary fix-up
    gots = chunked_runs(chain, x, case)
    if case.name == "disc-lds2-d50":
        # the tuner as ONE fused chain (what TunerBlock runs), then the discriminator block
        tun = lr.Chain(build(_tuner_specs(case), types.ComplexFloat32, rate))
        o = tun.process(x)
        want = make(lr.FrequencyDiscriminatorBlock, [A.GAIN], types.ComplexFloat32, rate / case.D).process(o)
    else:
        want, o = one_by_one(build(_tuner_specs(case, True), types.ComplexFloat32, rate), x)
    for got in gots:
        _compare_discriminator_epilogue(case, whole, got, want, o)


def _compare_discriminator_epilogue(case, whole, got, want, o):
    """one chunked run `got` of test_discriminator_epilogue against the unfused device blocks (`want`, their filter outputs `o`) and the oracle"""
    assert len(got) == len(whole) == len(want) == (case.n + case.D - 1) // case.D
    if case.bar == A.BITS:
        assert np.array_equal(whole, want) and np.array_equal(got, want)
    else:
        e = max(disc_err(whole, want, o, A.GAIN), disc_err(got, want, o, A.GAIN))
        _note("discriminator epilogue against the unfused device blocks", case.name, e, case.bar)
        assert e < case.bar
    # ... and the oracle chain with the same taps - the fused kernel and the unfused blocks read tap tables built by the same code, so the device alone
    # cannot show a table that both have mirrored.  The bars the existing tests hold their forms to: the median of the difference below 1e-6
    # (test_discriminator_epilogue_equals_unfused_blocks; reversed taps move the median above 1e-4, tests/test_asym_taps_cpu.py), and for the LDS form
    # disc_err() < 2e-6 (test_lds_staged_decimator_discriminator_epilogue)
    e = disc_err(got, ref(case), A.filter_output(case), A.GAIN)
    med = float(np.median(np.abs(got.astype(np.float64) - ref(case))))
    _note("discriminator epilogue against the oracle, disc_err", case.name, e, 2e-6)
    _note("discriminator epilogue against the oracle, median", case.name, med, 1e-6)
    if case.name == "disc-lds2-d50":
        assert e < 2e-6
    assert med < 1e-6


def test_discriminator_in_front():
    """plan_disc_fir: [FrequencyDiscriminator, FIR(random taps, "fast")] - 1e-6 against the oracle chain, two launches (test_discriminator_fir_chain_fusion)"""
    case, = [c for c in A.chain_cases() if c.group == "disc-front"]
    x, want = A.case_input(case), ref(case)

    def blocks():
        return build([(lr.FrequencyDiscriminatorBlock, [A.GAIN]), (lr.FIRFilterBlock, [case.taps[0], "fast"])], types.ComplexFloat32, 2.0)
    chain = lr.Chain(blocks())
    whole = chain.process(x)
    assert chain.last_launches == case.p["launches"]               # fused FFT kernel + history carry
    chain.reset()
    got = in_calls(chain, x, A.call_lengths(case.n, case.T, case.D))
    apart, _ = one_by_one(blocks(), x)
    assert len(got) == len(whole) == len(want) == case.n
    e = max(G.max_abs_err(whole, want), G.max_abs_err(got, want))
    _note("discriminator in front against the oracle", case.name, e, case.bar)
    _note("discriminator in front against the unfused device blocks", case.name, G.max_abs_err(got, apart), case.bar)
    assert e < case.bar and G.max_abs_err(got, apart) < case.bar


def test_unary_fold():
    """[FIR(77), Downsampler(18), ComplexMagnitude]: the magnitude runs on the LDS-staged decimator's accumulators - one launch, the bits of the unfused device
    blocks, and abs() of the fmaf-chain oracle at ComplexMagnitudeBlock's own bar"""
    case, = [c for c in A.chain_cases() if c.group == "unary"]
    x, want = A.case_input(case), ref(case)

    def blocks():
        return build([(lr.FIRFilterBlock, [case.taps[0]]), (lr.DownsamplerBlock, [case.D]), (lr.ComplexMagnitudeBlock, [])], types.ComplexFloat32, 2.0)
    chain = lr.Chain(blocks())
    whole = chain.process(x)
    assert chain.last_launches == case.p["launches"]
    chain.reset()
    got = in_calls(chain, x, A.call_lengths(case.n, case.T, case.D))
    apart, _ = one_by_one(blocks(), x)
    assert len(got) == len(want)
    assert np.array_equal(whole, apart) and np.array_equal(got, apart)
    eps = G.load("complexmagnitude_spec")["epsilon"]
    _note("unary fold against the oracle", case.name, G.max_abs_err(got, want), eps)
    assert G.max_abs_err(got, want) < eps


TAILS = [c for c in A.chain_cases() if c.group == "tail"]


@pytest.mark.parametrize("case", TAILS, ids=_ids(TAILS))
def test_polyphase_tail(case):
    """[FIR(h, "auto"), FMDeemphasisFilter, Downsampler(D)] -> the decimating filter g = h * b * (1, p, .., p^(D-1)) of plan_polyphase_tail: the bars and launch
    counts of test_fir_iir_downsampler_fused_vs_oracle_and_unfused"""
    x, want = A.case_input(case), ref(case)
    rate = case.p["rate"]
    chain = lr.Chain(build([(lr.FIRFilterBlock, [case.taps[0], "auto"]), (lr.FMDeemphasisFilterBlock, [case.p["tau"]]), (lr.DownsamplerBlock, [case.D])],
                           types.Float32, rate))
    whole = chain.process(x)
    lo, hi = case.p["launches_range"]
    assert lo <= chain.last_launches <= hi, chain.last_launches
    for got in chunked_runs(chain, x, case):
        assert len(got) == len(whole) == len(want)
        e = max(G.max_abs_err(whole, want), G.max_abs_err(got, want))
        _note("polyphase tail against the oracle", case.name, e, case.bar)
        _note("polyphase tail chunked against whole", case.name, G.max_abs_err(got, whole), 5e-7)
        assert e < case.bar and G.max_abs_err(got, whole) < 5e-7


RXS = [c for c in A.chain_cases() if c.group == "rx"]


@pytest.mark.parametrize("case", RXS, ids=_ids(RXS))
def test_receiver(case):
    """the WBFM receiver's chain with skewed taps in both filters: ONE launch (kernels_rx.h) by default, two with CHAIN_NO_SINGLE_LAUNCH; the bar of
    test_wbfm_receiver_launch_forms against the same chain built from oracle stages"""
    p = case.p
    x, want = A.case_input(case), ref(case)
    blocks = build([(lr.FrequencyTranslatorBlock, [p["offset"]]), (lr.FIRFilterBlock, [case.taps[0]]), (lr.DownsamplerBlock, [5]),
                    (lr.FrequencyDiscriminatorBlock, [A.GAIN]), (lr.FIRFilterBlock, [case.taps[1], "auto"]), (lr.FMDeemphasisFilterBlock, [p["tau"]]),
                    (lr.DownsamplerBlock, [5])], types.ComplexFloat32, p["rate"])
    chain = lr.Chain(blocks, _lib.CHAIN_NO_SINGLE_LAUNCH if p["launches"] == 2 else False)
    got = at_cuts(chain, x, p["cuts"])
    assert chain.last_launches == p["launches"]
    assert len(got) == len(want)
    err = got.astype(np.float64) - want.astype(np.float64)
    rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.max(np.abs(err)))
    _note("receiver rms", case.name, rms, case.bar[0])
    _note("receiver max", case.name, mx, case.bar[1])
    assert rms <= case.bar[0] and mx < case.bar[1]


# ===================================================================================================== C. resampler
RESAMPLERS = A.resample_cases()


@pytest.mark.parametrize("case", RESAMPLERS, ids=_ids(RESAMPLERS))
def test_resampler(case):
    """[MultiplyConstant(c)] -> Upsampler(L) -> FIR(random taps) -> [Downsampler(D)]: the bits of the zero-stuffed definition computed on the host (one
    Float32 product, then the fmaf chain over the zero-stuffed stream, every D-th output), whole and on ragged calls; one launch whenever the chain fuses"""
    p = case.p
    x, want = A.case_input(case), ref(case)
    specs = ([(lr.MultiplyConstantBlock, [p["c"]])] if p["c"] != 1.0 else []) + [(lr.UpsamplerBlock, [p["L"]]), (lr.FIRFilterBlock, [case.taps[0]])]
    if case.D > 1:
        specs.append((lr.DownsamplerBlock, [case.D]))
    chain = lr.Chain(build(specs, tp(case), 2.0))
    whole = chain.process(x)
    if p["fused"]:
        assert chain.last_launches == 1
    else:
        assert chain.last_launches > 1
    chain.reset()
    got = at_cuts(chain, x, A.RESAMPLE_CUTS)
    assert len(got) == len(whole) == len(want) == (case.n * p["L"] + case.D - 1) // case.D
    assert np.array_equal(whole, want), float(np.max(np.abs(whole - want)))
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
