"""IIRFilterBlock's kernel forms: a float64 restatement of the host rule that picks them, well-conditioned filters that reach each of
them, and the table of cases that tests/test_iir_forms_cpu.py (coverage, conditioning) and tests/test_gpu_iir_forms.py (values) share.

lrhip_iir_create (lrhip.hip) and IirStage::run_scan_nb (stage_iir.h) choose, from the taps alone:

    seq        iir_seq_kernel: no feedback taps, more than 8 of them, or more than 16 feed-forward taps
    oneshot    iir_stream_kernel, a workgroup per tile behind a PARTIAL warm-up tile of `warm_chunks` 16-sample chunks
    stream     iir_stream_kernel behind `warm_tiles` (1, 2 or 4) WHOLE warm-up tiles
    threepass  iir_scan_kernel twice around iir_tseg_kernel / iir_carry_kernel (and iir_state_kernel where nb > 1)

and, from the tap counts, the scan (first order: scalar wave scan; 2-4: matrix wave scan in Float32; 5-8: LDS Kogge-Stone in double), the
unroll bound NBT of the feed-forward loop and, in iir_stream_kernel, which of its compile-time tap counts is taken.  iir_form() says
which; the GPU tests hold it to what the library launched (one launch or several)."""
import collections
import functools
import math

import numpy as np

LC, TILE = 16, 4096                      # kernels_iir.h IIR_LC, IIR_TILE
MAX_P, MAX_NB, SEQ_MAX = 8, 16, 32       # IIR_MAX_P, IIR_MAX_NB, IIR_SEQ_MAX

# call lengths of the value tests: around a chunk, around a tile, then the smallest call that takes run = 2 * warm_tiles = 8 tiles per
# workgroup (more than 4 * 4 tiles), then a tail shorter than any order's state hand-over
CUTS = [1, 2, 15, 16, 17, 4095, 4096, 4097, 17 * TILE + 5, 3]
LARGEST = CUTS.index(17 * TILE + 5)
N_STREAM = sum(CUTS)
# constant 1.0 for five tiles, three silent tiles, 1.0 again: behind the silence a warm-up tile starts from zero where the true state is
# the decaying DC response
DC_CUTS = [3, 10 * TILE + 2]
N_DC = sum(DC_CUTS)


def _matpow2(M, squarings):
    for _ in range(squarings):
        M = M @ M
    return M


def iir_form(b, a):
    """(form, P, NBT, ff_specialisation, warm_tiles, warm_chunks) of IIRFilterBlock(b, a), as lrhip_iir_create decides it.
    NBT and ff_specialisation are None for the sequential kernel; the three-pass kernels always run the predicated loop."""
    b = np.asarray(b, np.float32)
    a = np.asarray(a, np.float32)
    nb, P = len(b), len(a) - 1
    if not (1 <= P <= MAX_P and nb <= MAX_NB):
        return ("seq", P, None, None, 0, 0)
    # IirCoeffs: taps over a[0] in double, rounded to Float32
    an = (a[1:].astype(np.float64) / float(a[0])).astype(np.float32).astype(np.float64)
    A = np.zeros((P, P))
    A[0, :] = -an
    for r in range(1, P):
        A[r, r - 1] = 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        A16 = _matpow2(A, 4)
        Ttile = _matpow2(A16, 8)
        warm_chunks = 0
        if P == 1:
            p16 = A16[0, 0]
            if abs(p16) < 1.0 and p16 != 0.0:
                wc = int(math.ceil(math.log(1e-12) / math.log(abs(p16))))
                if 1 <= wc <= 128:
                    warm_chunks = wc
            elif p16 == 0.0:
                warm_chunks = 1
        elif P <= 4:
            M = A16.copy()
            for wc in range(1, 129):
                mx = np.max(np.abs(M))
                if np.isfinite(mx) and mx < 1e-12:
                    warm_chunks = wc
                    break
                M = M @ A16
        warm_tiles = 0
        W = Ttile.copy()
        for w in (1, 2, 4):
            if np.all(np.isfinite(W)) and np.max(np.abs(W)) < 1e-46:
                warm_tiles = w
                break
            W = W @ W
    NBT = 2 if nb <= 2 else 4 if nb <= 4 else 8 if (P <= 4 and nb <= 8) else 16
    if warm_tiles == 0:
        return ("threepass", P, NBT, "predicated", 0, warm_chunks)
    d = NBT - nb
    spec = "NBT" if d == 0 else "NBT-1" if d == 1 else "NBT-%d" % d if (d in (2, 3) and NBT <= 8) else "predicated"
    return ("oneshot" if warm_chunks else "stream", P, NBT, spec, warm_tiles, warm_chunks)


def cell_of(form):
    """the form cell of the coverage table: whole-tile stream launches are told apart by their warm-up length"""
    return "stream%d" % form[4] if form[0] == "stream" else form[0]


# --------------------------------------------------------------------------------------------------------- filters
def placed_poles(P, r, lo=0.4, hi=2.7):
    """well-separated poles: conjugate pairs on radius r at angles linspace(lo, hi), and for odd orders a real pole at -r / 2.
    First order is the single real pole r itself (FIRST_ORDER_POLES)."""
    if P == 1:
        return [complex(r)]
    ang = np.linspace(lo, hi, P // 2)
    return list(r * np.exp(1j * ang)) + list(r * np.exp(-1j * ang)) + ([-0.5 * r] if P % 2 else [])


def placed_filter(P, r, nb, seed, a0=1.0, lo=0.4, hi=2.7):
    """(b, a) in Float32: feedback taps from placed_poles, nb feed-forward taps 0.1 * U(-1, 1); a0 scales every tap (exactly, for powers
    of two)"""
    rng = np.random.default_rng(seed)
    a = np.real(np.poly(placed_poles(P, r, lo, hi))) if P else np.ones(1)
    b = 0.1 * rng.uniform(-1, 1, nb)
    return (b * a0).astype(np.float32), (a * a0).astype(np.float32)


# --------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "name group cplx b a radius seed kind n expect")
# kind: "stream" (uniform data, host calls), "dc" (the on / off / on input over DC_CUTS), "long" (uniform data, device calls)
# radius: the placement's radius (1.0 = poles on the unit circle: the wider conditioning limit)
# expect: (form, warm_tiles) where the tables below state it, else None


def make_case(group, cplx, P, r, nb, seed, kind="stream", n=None, expect=None, a0=1.0, lo=0.4, hi=2.7):
    b, a = placed_filter(P, r, nb, seed, a0, lo, hi)
    n = n if n is not None else (N_DC if kind == "dc" else N_STREAM)
    return Case("%s-%s-P%d-r%s-nb%d%s" % (group, "cf32" if cplx else "f32", P, ("%g" % r), nb, "" if a0 == 1.0 else "-a0=%g" % a0) +
                ("" if kind == "stream" else "-" + kind), group, cplx, b, a, abs(r), seed, kind, n, expect)


FIRST_ORDER_POLES = [(0.0, ("oneshot", 1)), (0.5, ("oneshot", 1)), (-0.9, ("oneshot", 1)), (0.97, ("oneshot", 1)), (0.9868, ("stream", 2)),
                     (0.99, ("stream", 4)), (0.9995, ("threepass", 0)), (1.0, ("threepass", 0))]


def _expect(P, r):
    if r >= 0.9995:
        return ("threepass", 0)
    if r == 0.99:
        return ("stream", 4)
    if P <= 4:
        return ("oneshot", 1 if r == 0.85 else 2)
    return ("stream", 1 if r == 0.85 else 2)


RADII = [0.85, 0.986, 0.99, 0.9995, 1.0]
# orders 2-4 behind two WHOLE warm-up tiles: the narrow window (0.9865 .. 0.9871 with this placement) in which A^8192 is below 1e-46
# while A^2048 is still above 1e-12, as the first-order pole 0.9868 is; tests/test_iir_forms_cpu.py holds it to the rule
STREAM2_RADIUS = 0.9868


@functools.lru_cache(maxsize=None)
def form_cross_cases():
    """every reachable (stream type, order, form) cell, three feed-forward taps; the single-launch forms a second time on the DC input"""
    out, seed = [], 7000
    for cplx in (False, True):
        for pole, exp in FIRST_ORDER_POLES:
            seed += 1
            out.append(make_case("cross", cplx, 1, pole, 3, seed, expect=exp))
            if exp[0] != "threepass":
                out.append(make_case("cross", cplx, 1, pole, 3, seed, kind="dc", expect=exp))
        for P in range(2, MAX_P + 1):
            for r in RADII + ([STREAM2_RADIUS] if P <= 4 else []):
                seed += 1
                exp = ("stream", 2) if r not in RADII else _expect(P, r)
                out.append(make_case("cross", cplx, P, r, 3, seed, expect=exp))
                if exp[0] != "threepass":
                    out.append(make_case("cross", cplx, P, r, 3, seed, kind="dc", expect=exp))
    return tuple(out)


SWEEP_NB = [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 15, 16]
SWEEP_P = [1, 2, 4, 5, 8]


@functools.lru_cache(maxsize=None)
def tap_sweep_cases():
    """every NBT and every compile-time tap count of iir_stream_kernel (radius 0.85), the same tap counts through the three-pass
    kernels (0.9995), and one filter given with a[0] = 2 and every tap doubled"""
    out, seed = [], 8000
    for cplx in (False, True):
        for P in SWEEP_P:
            for r in (0.85, 0.9995):
                for nb in SWEEP_NB:
                    seed += 1
                    out.append(make_case("sweep", cplx, P, r, nb, seed))
    out.append(make_case("sweep", True, 4, 0.85, 5, 8999, a0=2.0))
    out.append(make_case("sweep", False, 5, 0.9995, 6, 8998, a0=2.0))
    return tuple(out)


SEQ_SHAPES = [(3, 1, 1.0), (1, 1, 2.5), (3, 10, 1.0), (17, 3, 1.0), (32, 32, 1.0)]      # (nb, na, a[0])
SEQ_CUTS = [1, 40, 5000]


@functools.lru_cache(maxsize=None)
def seq_cases():
    """iir_seq_kernel by its three routes: no feedback taps, more than 8, more than 16 feed-forward taps"""
    out, seed = [], 9000
    for cplx in (False, True):
        for nb, na, a0 in SEQ_SHAPES:
            seed += 1
            out.append(make_case("seq", cplx, na - 1, 0.8, nb, seed, n=sum(SEQ_CUTS), a0=a0, lo=0.2, hi=2.9))
    return tuple(out)


CARRY_P = [1, 3, 4, 5, 8]
CARRY_CALLS = [257 * TILE + 5, 513 * TILE + 5]      # seg = ceil(ntiles / 256) = 2, then 3 (odd: the e & 1 branch of iir_tseg_kernel)


@functools.lru_cache(maxsize=None)
def carry_cases():
    out, seed = [], 9100
    for cplx in (False, True):
        for P in CARRY_P:
            seed += 1
            out.append(make_case("carry", cplx, P, 0.9995, 3, seed, kind="long", n=sum(CARRY_CALLS)))
        seed += 1
        out.append(make_case("carry", cplx, 4, 1.0, 3, seed, kind="long", n=sum(CARRY_CALLS)))
    return tuple(out)


def run2_cases(cus):
    """one-shot form at two tiles per workgroup (Float32): first order from 8 tiles per CU on, orders 2-4 from 16"""
    return (make_case("run2", False, 1, 0.5, 3, 9201, kind="long", n=8 * cus * TILE + 5, expect=("oneshot", 1)),
            make_case("run2", False, 2, 0.85, 3, 9202, kind="long", n=16 * cus * TILE + 5, expect=("oneshot", 1)))


MISALIGNED_CALLS = [2 * TILE + 1, 3]


@functools.lru_cache(maxsize=None)
def misaligned_cases():
    out = []
    for cplx in (False, True):
        out.append(make_case("misaligned", cplx, 2, 0.85, 3, 9301 + cplx, kind="long", n=sum(MISALIGNED_CALLS), expect=("oneshot", 1)))
        out.append(make_case("misaligned", cplx, 5, 0.85, 3, 9303 + cplx, kind="long", n=sum(MISALIGNED_CALLS), expect=("stream", 1)))
        out.append(make_case("misaligned", cplx, 3, 0.9995, 3, 9305 + cplx, kind="long", n=sum(MISALIGNED_CALLS), expect=("threepass", 0)))
    return tuple(out)


def value_cases(cus=256):
    """every case whose values a GPU test compares with the f64 recurrence (the conditioning check runs over all of them)"""
    return form_cross_cases() + tap_sweep_cases() + seq_cases() + carry_cases() + run2_cases(cus) + misaligned_cases()


# --------------------------------------------------------------------------------------------------------- inputs, reference, bar
def case_input(case):
    rng = np.random.default_rng(case.seed + 100000)
    if case.kind == "dc":
        x = np.zeros(case.n, np.float32)
        x[:5 * TILE] = 1.0
        x[8 * TILE:] = 1.0
        return (x * np.complex64(1.0 - 0.5j)).astype(np.complex64) if case.cplx else x
    if case.cplx:
        x = np.empty(case.n, np.complex64)
        v = x.view(np.float32)
        v[:] = rng.uniform(-1, 1, 2 * case.n).astype(np.float32)
        return x
    return rng.uniform(-1, 1, case.n).astype(np.float32)


def case_cuts(case):
    """the call lengths the case's stream is fed in"""
    if case.kind == "dc":
        return DC_CUTS
    cuts = {"seq": SEQ_CUTS, "carry": CARRY_CALLS, "misaligned": MISALIGNED_CALLS, "run2": [case.n]}.get(case.group, CUTS)
    assert sum(cuts) == case.n, case.name
    return cuts


def reference(case, x=None):
    """(x, want, yard, scale): the f64 recurrence over the whole stream, what the reference's own sequential Float32 recurrence loses
    against it, and the output's scale"""
    from oracle import oracle as O
    x = case_input(case) if x is None else x
    want = O.IIR(case.b, case.a, case.cplx, O.MODE_F64).process(x)
    lua = O.IIR(case.b, case.a, case.cplx, O.MODE_LUA).process(x)
    yard = float(np.max(np.abs(lua.astype(np.complex128 if case.cplx else np.float64) - want))) if len(x) else 0.0
    scale = max(1.0, float(np.max(np.abs(want))))
    return x, want, yard, scale


def conditioning_limit(case, scale):
    return (1e-4 if case.radius >= 1.0 else 1e-5) * scale


def bar(yard, scale):
    """test_iir_orders_five_to_eight_scan_paths: at most ten times the sequential Float32 recurrence's own loss, plus 2e-6 of the scale"""
    return 10 * yard + 2e-6 * scale
