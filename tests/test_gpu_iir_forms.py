"""IIRFilterBlock on every kernel form it dispatches (tests/helpers/iir_forms.py has the forms, the filters that reach them and the case
table; tests/test_iir_forms_cpu.py holds the table to its coverage and to its conditioning), against the f64 recurrence over the whole
stream.

Bar, everywhere a value is compared: that of test_iir_orders_five_to_eight_scan_paths, max|got - want| <= 10 * yard + 2e-6 * scale, with
yard what the reference's own sequential Float32 recurrence loses against f64 on the same input (at most 1e-5 of the scale by the
conditioning check, 1e-4 on the unit circle) and scale = max(1, max|want|); equal lengths; no non-finite output.  Every block of the form
cross, the tap-count sweep and the sequential cases runs as a one-stage unfused chain, whose launch count after the largest call must be
what iir_form() says of the filter: 1 for the one-shot, stream and sequential forms, 2 or more for the three-pass form."""
import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests.helpers import iir_forms as F

pytestmark = pytest.mark.gpu


def make_iir(case):
    blk = lr.IIRFilterBlock(case.b, case.a)
    blk.rate = 2.0
    blk.differentiate([types.ComplexFloat32 if case.cplx else types.Float32])
    blk.initialize()
    return blk


def make_ds(factor, cplx):
    blk = lr.DownsamplerBlock(factor)
    blk.rate = 2.0
    blk.differentiate([types.ComplexFloat32 if cplx else types.Float32])
    blk.initialize()
    return blk


def calls(obj, x, cuts):
    parts, s = [], 0
    for n in cuts:
        parts.append(obj.process(x[s:s + n]))
        s += n
    assert s == len(x)
    return np.concatenate(parts)


def ratio(case, got, want, yard, scale):
    """err / bar after the checks on length and finiteness; the caller asserts <= 1 (and keeps the largest for the report)"""
    assert len(got) == len(want), (case.name, len(got), len(want))
    assert np.all(np.isfinite(got.view(np.float32))), case.name
    err = float(np.max(np.abs(got.astype(np.complex128 if case.cplx else np.float64) - want))) if len(want) else 0.0
    return err / F.bar(yard, scale), err


def run_unfused_chain(case, x):
    """the block as a one-stage chain without fusion: (output, launches of the largest call)"""
    blk = make_iir(case)
    chain = lr.Chain([blk], exact=_lib.CHAIN_NO_FUSION)
    cuts = F.case_cuts(case)
    parts, s, launches = [], 0, None
    for n in cuts:
        parts.append(chain.process(x[s:s + n]))
        if n == max(cuts):
            launches = chain.last_launches
        s += n
    assert s == len(x) and launches is not None
    return np.concatenate(parts), launches


def check_cases(cases):
    worst, bad = (0.0, None), []
    for case in cases:
        x, want, yard, scale = F.reference(case)
        got, launches = run_unfused_chain(case, x)
        form = F.iir_form(case.b, case.a)
        # the Python restatement of the host rule against what the library launched
        if form[0] == "threepass":
            assert launches >= 2, (case.name, form, launches)
        else:
            assert launches == 1, (case.name, form, launches)
        r, err = ratio(case, got, want, yard, scale)
        worst = max(worst, (r, case.name))
        if not r <= 1.0:
            bad.append("%s %s: err %.3g, yard %.3g, scale %.3g, err / bar %.3g" % (case.name, form, err, yard, scale, r))
    print("worst err / (10 * yard + 2e-6 * scale): %.3g (%s)" % worst)
    assert not bad, "\n".join(bad)


def _order(case):
    return len(case.a) - 1


# ------------------------------------------------------------------------------------------------------------- 1-3
@pytest.mark.parametrize("P", range(1, F.MAX_P + 1))
@pytest.mark.parametrize("cplx", [False, True])
def test_form_cross(cplx, P):
    """every reachable (stream type, order, form) cell with three feed-forward taps, on uniform data over the ragged calls and, for the
    single-launch forms, on the on / off / on input whose warm-up tiles start from zero while the true state decays from the DC gain"""
    cases = [c for c in F.form_cross_cases() if c.cplx == cplx and _order(c) == P]
    assert {c.kind for c in cases} == {"stream", "dc"}
    check_cases(cases)


@pytest.mark.parametrize("P", F.SWEEP_P)
@pytest.mark.parametrize("cplx", [False, True])
def test_tap_count_sweep(cplx, P):
    """every unroll bound NBT and every compile-time tap count of iir_stream_kernel (radius 0.85), the same counts through the
    three-pass kernels (0.9995); a[0] = 2 with every tap doubled is the same filter and is held to the same bar"""
    cases = [c for c in F.tap_sweep_cases() if c.cplx == cplx and _order(c) == P]
    assert len(cases) >= 2 * len(F.SWEEP_NB)
    check_cases(cases)


# ------------------------------------------------------------------------------------------------------------- 4-6: device calls
def _to_device(x):
    import torch
    return torch.from_numpy(x.view(np.float32)).cuda()


def _device_calls(case, x, cuts, in_off=0, out_off=0):
    """each call from its own torch allocation (16-byte aligned and more), moved by in_off / out_off SAMPLES"""
    import torch
    blk = make_iir(case)
    w = 2 if case.cplx else 1
    parts, s = [], 0
    for n in cuts:
        xt = torch.empty((n + 1) * w, dtype=torch.float32, device="cuda")
        xt[in_off * w:(in_off + n) * w] = _to_device(np.ascontiguousarray(x[s:s + n]))
        yt = torch.full(((n + 2) * w,), np.nan, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert xt.data_ptr() % 16 == 0 and yt.data_ptr() % 16 == 0
        got_n = blk.process_device(xt.data_ptr() + in_off * w * 4, n, yt.data_ptr() + out_off * w * 4, n)
        _lib.load().lrhip_synchronize()
        assert got_n == n
        y = yt.cpu().numpy()
        # nothing in front of the output or behind it is written
        assert np.all(np.isnan(y[:out_off * w])) and np.all(np.isnan(y[(out_off + n) * w:])), (case.name, n)
        y = y[out_off * w:(out_off + n) * w]
        parts.append(y.view(np.complex64) if case.cplx else y)
        s += n
    return np.concatenate(parts)


@pytest.mark.parametrize("case", F.carry_cases(), ids=lambda c: c.name)
def test_carry_scan_across_segments(case):
    """three-pass filters on single calls of 257 and then 513 tiles and 5 samples: iir_carry_kernel with seg = 2 and 3 tiles per thread,
    iir_tseg_kernel's squaring with an even and an odd exponent (the smallest lengths that do; the host path would cut such a call into
    pieces, so the calls are device calls)"""
    assert F.iir_form(case.b, case.a)[0] == "threepass"
    x, want, yard, scale = F.reference(case)
    got = _device_calls(case, x, F.CARRY_CALLS)
    r, err = ratio(case, got, want, yard, scale)
    print("err / bar %.3g (err %.3g, yard %.3g, scale %.3g)" % (r, err, yard, scale))
    assert r <= 1.0, (case.name, err, yard, scale)


@pytest.mark.parametrize("which", [0, 1], ids=["first-order-8-tiles-per-cu", "order-2-16-tiles-per-cu"])
def test_one_shot_form_two_tiles_per_workgroup(which):
    """the one-shot launch gives a workgroup two tiles from 8 tiles per CU on at first order and from 16 on at orders 2-4 (more than
    two need 2^26 samples and are left out)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = F.run2_cases(cus)[which]
    if case.n > 1 << 25:
        pytest.skip("%d CUs: %d samples is more than 2^25" % (cus, case.n))
    assert F.iir_form(case.b, case.a)[0] == "oneshot"
    x, want, yard, scale = F.reference(case)
    got = _device_calls(case, x, [case.n])
    r, err = ratio(case, got, want, yard, scale)
    print("err / bar %.3g (err %.3g, yard %.3g, scale %.3g)" % (r, err, yard, scale))
    assert r <= 1.0, (case.name, err, yard, scale)


@pytest.mark.parametrize("case", F.misaligned_cases(), ids=lambda c: c.name)
def test_misaligned_device_pointers(case):
    """input, output or both only sample-aligned (4 / 8 bytes): the scalar load and store paths of each form"""
    assert tuple(F.iir_form(case.b, case.a)[0::4]) == case.expect
    x, want, yard, scale = F.reference(case)
    for in_off, out_off in ((1, 0), (0, 1), (1, 1)):
        got = _device_calls(case, x, F.MISALIGNED_CALLS, in_off, out_off)
        r, err = ratio(case, got, want, yard, scale)
        assert r <= 1.0, (case.name, in_off, out_off, err, yard, scale)


# ------------------------------------------------------------------------------------------------------------- 7: fused downsampler
DS_CUTS = [(0, 1), (1, 2), (2, 4097), (4097, 4098), (4098, 50000), (50000, 90001)]       # test_iir_downsampler_chain_fusion's
DS_RADII = {"short": 0.85, "stream": 0.99, "threepass": 0.9995}      # 0.85: one-shot at orders 1 and 2, one whole warm-up tile at order 5


@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("which", sorted(DS_RADII))
@pytest.mark.parametrize("cplx", [False, True])
def test_fused_downsampler_on_every_form(cplx, which, P):
    """[IIR -> Downsampler] stores only the kept samples, in iir_stream_kernel and in the FINAL pass of iir_scan_kernel: the same bits
    as the two blocks one after the other over the same calls, one launch less"""
    n = DS_CUTS[-1][1]
    case = F.make_case("ds", cplx, P, DS_RADII[which], 3, 9400 + P, n=n)
    form = F.iir_form(case.b, case.a)
    assert F.cell_of(form) == {"short": "stream1" if P > 4 else "oneshot", "stream": "stream4", "threepass": "threepass"}[which]
    x = F.case_input(case)
    ref_iir = make_iir(case)
    filtered = [ref_iir.process(x[a:b]) for a, b in DS_CUTS]
    for factor in (2, 5, 16, 17, 4096, 5000):
        iir, ds = make_iir(case), make_ds(factor, cplx)
        chain = lr.Chain([iir, ds])
        got = np.concatenate([chain.process(x[a:b]) for a, b in DS_CUTS])
        ref_ds = make_ds(factor, cplx)
        want = np.concatenate([ref_ds.process(f) for f in filtered])
        assert len(got) == (n + factor - 1) // factor, (factor, len(got))
        assert np.array_equal(got, want), (case.name, factor)
        i2, d2 = make_iir(case), make_ds(factor, cplx)
        apart = lr.Chain([i2, d2], exact=_lib.CHAIN_NO_FUSION)
        apart.process(x[50000:n])
        assert chain.last_launches < apart.last_launches, (case.name, factor, chain.last_launches, apart.last_launches)


@pytest.mark.parametrize("cplx", [False, True])
def test_sequential_filter_is_not_fused_with_a_downsampler(cplx):
    """iir_seq_kernel stores every sample (it ignores D): plan_iir_downsample must leave a ninth-order filter and its downsampler apart"""
    n = DS_CUTS[-1][1]
    case = F.make_case("ds", cplx, 9, 0.8, 3, 9450, n=n, lo=0.2, hi=2.9)
    assert F.iir_form(case.b, case.a)[0] == "seq"
    x = F.case_input(case)
    for factor in (2, 17, 5000):
        iir, ds = make_iir(case), make_ds(factor, cplx)
        chain = lr.Chain([iir, ds])
        got = np.concatenate([chain.process(x[a:b]) for a, b in DS_CUTS])
        ref_iir, ref_ds = make_iir(case), make_ds(factor, cplx)
        want = np.concatenate([ref_ds.process(ref_iir.process(x[a:b])) for a, b in DS_CUTS])
        assert len(got) == (n + factor - 1) // factor
        assert np.array_equal(got, want), factor
        i2, d2 = make_iir(case), make_ds(factor, cplx)
        apart = lr.Chain([i2, d2], exact=_lib.CHAIN_NO_FUSION)
        apart.process(x[50000:n])
        assert chain.last_launches == apart.last_launches, (factor, chain.last_launches, apart.last_launches)


# ------------------------------------------------------------------------------------------------------------- 8: sequential kernel
@pytest.mark.parametrize("cplx", [False, True])
def test_sequential_kernel(cplx):
    """iir_seq_kernel by its three routes (no feedback taps, more than 8, more than 16 feed-forward taps), up to the 32 + 32 taps it holds"""
    cases = [c for c in F.seq_cases() if c.cplx == cplx]
    assert [(len(c.b), len(c.a)) for c in cases] == [(nb, na) for nb, na, _ in F.SEQ_SHAPES]
    check_cases(cases)


@pytest.mark.parametrize("b,a,message", [(np.ones(33), np.ones(1), "iir: at most 32 taps supported"), (np.ones(1), [1.0] + [0.0] * 32, "iir: at most 32 taps supported"),
                                         (np.ones(2), [0.0, 0.5], "iir: a[0] must be non-zero")])
def test_refused_tap_counts(b, a, message):
    blk = lr.IIRFilterBlock(np.asarray(b, np.float32), np.asarray(a, np.float32))
    blk.rate = 2.0
    blk.differentiate([types.Float32])
    with pytest.raises(_lib.LrhipError) as e:
        blk.initialize()
    assert message in str(e.value)


# ------------------------------------------------------------------------------------------------------------- 9: reset
RESET_CASES = [F.make_case("reset", False, 2, 0.85, 3, 9501, expect=("oneshot", 1)), F.make_case("reset", False, 6, 0.986, 5, 9502, expect=("stream", 2)),
               F.make_case("reset", True, 7, 0.9995, 3, 9503, expect=("threepass", 0)), F.make_case("reset", True, 9, 0.8, 3, 9504, lo=0.2, hi=2.9, expect=("seq", 0))]


@pytest.mark.parametrize("case", RESET_CASES, ids=lambda c: c.name)
def test_reset_restores_the_initial_state(case):
    assert tuple(F.iir_form(case.b, case.a)[0::4]) == case.expect
    x = F.case_input(case)
    blk = make_iir(case)
    first = calls(blk, x, F.CUTS)
    blk.reset()
    again = calls(blk, x, F.CUTS)
    assert len(first) == len(x) and np.array_equal(first, again)
    # and a stream cut short leaves nothing behind either
    blk.process(x[:4099])
    blk.reset()
    assert np.array_equal(calls(blk, x, F.CUTS), first)
