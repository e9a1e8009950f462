"""The case table of tests/test_gpu_asym_taps.py (tests/helpers/asym_taps.py), checked where no GPU is needed.  Conditions on the inputs, not
measurements of the kernels: every case's reference moves by at least 0.02 of its rms when the taps are reversed (and is not the same bits where the
bar is bit equality), so a kernel or a tap table that walks the taps backwards cannot pass; the table reaches every (form, stream type) pair it is
there for; and the one-launch receiver's reference does not eat the bar - its MODE_LUA and MODE_F64 evaluations agree to a tenth of it."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import asym_taps as A

MIN_MOVE = 0.02


def missing_forms(cases):
    have = {(c.form, c.stream) for c in cases}
    return ["no case for %s on %s" % f for f in A.FORMS if f not in have] + ["%s on %s is not in the form list" % f for f in sorted(have) if f not in A.FORMS]


def test_case_table_covers_every_form():
    cases = A.all_cases()
    assert not missing_forms(cases), "\n".join(missing_forms(cases))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)


def test_a_removed_form_is_named():
    """the coverage check is not vacuous"""
    cases = A.all_cases()
    assert missing_forms([c for c in cases if c.form != "WinPair"]) == ["no case for WinPair on f32"]
    assert missing_forms([c for c in cases if not (c.form == "resample" and c.stream == "cf32")]) == ["no case for resample on cf32"]
    assert missing_forms(cases + [cases[0]._replace(form="nonesuch")]) == ["nonesuch on cf32 is not in the form list"]


def test_taps_are_not_symmetric_and_their_ends_are_large():
    rng = np.random.default_rng(1)
    for M in (5, 13, 16, 33, 128, 256):
        h = A.random_taps(rng, M)
        assert h.dtype == np.float32 and len(h) == M and min(abs(h[0]), abs(h[-1])) >= 0.25 / M and not np.array_equal(h, h[::-1])
    for M, cutoff in ((128, 0.2), (77, 1 / 18), (64, 0.2), (128, 100e3 / (A.FS / 2))):
        h = A.skewed_lowpass(M, cutoff)
        assert h.dtype == np.float32 and abs(float(np.sum(h.astype(np.float64))) - 1.0) < 1e-6
        assert not np.array_equal(h, h[::-1])
    for c in A.all_cases():
        for h in c.taps:
            assert not np.array_equal(h, h[::-1]), c.name


def _groups():
    return sorted({c.group for c in A.all_cases()})


@pytest.mark.parametrize("group", _groups())
def test_reversed_taps_move_every_reference(group):
    bad, worst, seen = [], (np.inf, None), {}
    for c in A.all_cases():
        if c.group != group:
            continue
        key = (c.n, c.D, c.stream, tuple(h.tobytes() for h in c.taps), repr(sorted((k, v) for k, v in c.p.items() if k in ("rate", "offset", "L", "c", "use_fft", "tau"))),
               c.bar == A.BITS)
        if key in seen:          # the same reference as an earlier case (the receiver's two launch forms, the exact twin of a discriminator case)
            continue
        seen[key] = c.name
        want = A.reference(c)
        assert np.all(np.isfinite(want.view(np.float32))), c.name
        rms = float(np.sqrt(np.mean(np.abs(want.astype(np.complex128 if want.dtype.kind == "c" else np.float64)) ** 2)))
        for which in range(len(c.taps)):
            rev = A.reference(c, A.reversed_taps(c, which))
            assert len(rev) == len(want), c.name
            d = rev.astype(np.complex128 if rev.dtype.kind == "c" else np.float64) - want
            move = float(np.sqrt(np.mean(np.abs(d) ** 2))) / rms
            worst = min(worst, (move, "%s taps %d" % (c.name, which)))
            if move < MIN_MOVE or (c.bar == A.BITS and np.array_equal(rev, want)):
                bad.append("%s, taps %d: reversed taps move the reference by %.3g of its rms" % (c.name, which, move))
            # the discriminator cases are also held to the oracle in the median, at 1e-6: reversed taps must move the median a hundred times that
            if group == "disc" and float(np.median(np.abs(d))) < 1e-4:
                bad.append("%s: reversed taps move the median by %.3g only" % (c.name, float(np.median(np.abs(d)))))
    print("%s: smallest move %.3g of the rms (%s)" % (group, worst[0], worst[1]))
    assert not bad, "\n".join(bad)


def test_receiver_reference_does_not_eat_the_bar():
    """MODE_LUA (the reference's own Float32 arithmetic, what the GPU test compares with) against MODE_F64 on the case's input: a tenth of the GPU bar"""
    for c in A.all_cases():
        if c.group != "rx" or c.p["launches"] != 1:
            continue
        rms_bar, max_bar = c.bar
        err = A.reference(c, mode=O.MODE_LUA).astype(np.float64) - A.reference(c, mode=O.MODE_F64).astype(np.float64)
        rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.max(np.abs(err)))
        print("receiver reference: LUA against F64 rms %.3g (bar / 10 = %.3g), max %.3g (%.3g)" % (rms, rms_bar / 10, mx, max_bar / 10))
        assert rms <= rms_bar / 10 and mx < max_bar / 10


def test_stream_lengths_and_calls():
    for c in A.fir_cases() + [c for c in A.chain_cases() if c.group != "rx"]:
        assert c.n == 3 * c.T * c.D + c.T * c.D // 2 + 7, c.name
        calls = A.call_lengths(c.n, c.T, c.D)
        assert calls[0] == 1 and calls[1] == 2 * c.T * c.D + 3 and sum(calls) == c.n and min(calls) > 0, c.name
        assert A.chunkings(c)[0] == calls and len(A.chunkings(c)) == (2 if c.D >= 2 else 1), c.name
        if c.D >= 2:
            # the first call of 1 leaves the carried index at D - 1; a call of m samples emits only when m exceeds it
            idle = A.idle_call_lengths(c.n, c.T, c.D)
            assert idle[:3] == [1, 1, 2 * c.T * c.D + 3] and len(idle) == 4 and sum(idle) == c.n and min(idle) > 0 and idle[1] <= c.D - 1, c.name
