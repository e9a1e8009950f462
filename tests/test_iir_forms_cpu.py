"""The case table of tests/test_gpu_iir_forms.py, checked where no GPU is needed: it reaches every kernel form IIRFilterBlock can
dispatch (by tests/helpers/iir_forms.py's restatement of the host rule, which the GPU tests tie to the launches the library makes), and
every one of its filters is well conditioned - the reference's own sequential Float32 recurrence stays within 1e-5 of the output's scale
of the f64 one (1e-4 for poles on the unit circle) on the case's own input - so that the GPU bar, ten times that loss, cannot hide a
kernel's error."""
import numpy as np
import pytest

from tests.helpers import iir_forms as F

STREAMS = ("f32", "cf32")
CELLS = ("oneshot", "stream1", "stream2", "stream4", "threepass")

# cells of {stream type} x {order} x {form} that no filter reaches, with the reason
UNREACHABLE = {}
for _s in STREAMS:
    for _P in range(1, 5):
        UNREACHABLE[(_s, _P, "stream1")] = ("one whole warm-up tile means every entry of A^4096 is below 1e-46, so the spectral radius is below 0.975 and A^2048 "
                                            "is near 1e-23: the 1e-12 warm_chunks rule (at most 128 chunks = 2048 samples) fires first and the launch is one-shot")
    for _P in range(5, 9):
        UNREACHABLE[(_s, _P, "oneshot")] = "warm_chunks is only computed for orders 1-4 (lrhip_iir_create)"
# feed-forward specialisations of iir_stream_kernel that no tap count reaches
FF_UNREACHABLE = {(4, "NBT-2"): "nb = 2 takes NBT = 2", (4, "NBT-3"): "nb = 1 takes NBT = 2"}
FF_ALL = [(2, "NBT"), (2, "NBT-1"), (4, "NBT"), (4, "NBT-1"), (4, "NBT-2"), (4, "NBT-3"), (8, "NBT"), (8, "NBT-1"), (8, "NBT-2"), (8, "NBT-3"),
          (16, "NBT"), (16, "NBT-1"), (16, "predicated")]
SEQ_ROUTES = ("P = 0", "P > 8", "nb > 16")


def _stream(case):
    return "cf32" if case.cplx else "f32"


def missing_cells(cross, sweep, seq):
    """names of the cells the three tables leave out (and of unreachable cells they reach after all: then the list above is wrong)"""
    out = []
    reached = {(_stream(c), F.iir_form(c.b, c.a)[1], F.cell_of(F.iir_form(c.b, c.a))) for c in cross if c.kind == "stream"}
    dc = {(_stream(c), F.iir_form(c.b, c.a)[1], F.cell_of(F.iir_form(c.b, c.a))) for c in cross if c.kind == "dc"}
    for s in STREAMS:
        for P in range(1, F.MAX_P + 1):
            for cell in CELLS:
                key = (s, P, cell)
                if key in UNREACHABLE:
                    if key in reached:
                        out.append("form cross reaches %s, which is listed as unreachable" % (key,))
                    continue
                if key not in reached:
                    out.append("form cross: no case for %s" % (key,))
                if cell != "threepass" and key not in dc:
                    out.append("form cross: no DC-input case for %s" % (key,))
    for s in STREAMS:
        forms = [F.iir_form(c.b, c.a) for c in sweep if _stream(c) == s]
        single = {(f[2], f[3]) for f in forms if f[0] in ("oneshot", "stream")}
        for key in FF_ALL:
            if key in FF_UNREACHABLE:
                if key in single:
                    out.append("tap sweep reaches %s on %s, which is listed as unreachable" % (key, s))
            elif key not in single:
                out.append("tap sweep: no single-launch case for (NBT, specialisation) = %s on %s" % (key, s))
        for P in F.SWEEP_P:
            for form in ("single", "threepass"):
                nbt = {f[2] for f in forms if f[1] == P and (f[0] == "threepass") == (form == "threepass")}
                for want in (2, 4, 16) + ((8,) if P <= 4 else ()):
                    if want not in nbt:
                        out.append("tap sweep: no %s case with NBT = %d at order %d on %s" % (form, want, P, s))
        routes = set()
        for c in seq:
            f = F.iir_form(c.b, c.a)
            if _stream(c) == s and f[0] == "seq":
                routes |= {r for r, hit in zip(SEQ_ROUTES, (f[1] == 0, f[1] > F.MAX_P, len(c.b) > F.MAX_NB)) if hit}
        out += ["sequential kernel: no case by the route %s on %s" % (r, s) for r in SEQ_ROUTES if r not in routes]
    return out


def test_case_table_reaches_every_reachable_cell():
    missing = missing_cells(F.form_cross_cases(), F.tap_sweep_cases(), F.seq_cases())
    assert not missing, "\n".join(missing)


def test_a_removed_case_is_named():
    """the coverage check is not vacuous: take the only case of one cell out of each table and it says which cell is gone"""
    cross, sweep, seq = F.form_cross_cases(), F.tap_sweep_cases(), F.seq_cases()

    def gone(c):
        f = F.iir_form(c.b, c.a)
        return c.cplx and f[1] == 3 and F.cell_of(f) == "stream2" and c.kind == "stream"
    assert missing_cells([c for c in cross if not gone(c)], sweep, seq) == ["form cross: no case for ('cf32', 3, 'stream2')"]
    thin = [c for c in sweep if not (not c.cplx and len(c.b) == 5 and F.iir_form(c.b, c.a)[0] == "oneshot")]
    assert missing_cells(cross, thin, seq) == ["tap sweep: no single-launch case for (NBT, specialisation) = (8, 'NBT-3') on f32"]
    assert missing_cells(cross, sweep, [c for c in seq if len(c.b) <= F.MAX_NB]) == ["sequential kernel: no case by the route nb > 16 on %s" % s for s in STREAMS]


def test_cases_take_the_forms_the_tables_state():
    for c in F.form_cross_cases() + F.run2_cases(256) + F.misaligned_cases():
        f = F.iir_form(c.b, c.a)
        assert (f[0], f[4]) == c.expect, (c.name, f)
    for c in F.tap_sweep_cases():
        f = F.iir_form(c.b, c.a)
        assert (f[0] == "threepass") == (c.radius == 0.9995), (c.name, f)
        assert f[0] != "seq", c.name
    for c in F.carry_cases():
        assert F.iir_form(c.b, c.a)[0] == "threepass", c.name
    for c in F.seq_cases():
        assert F.iir_form(c.b, c.a)[0] == "seq", c.name
    names = [c.name for c in F.value_cases()]
    assert len(set(names)) == len(names)


def test_iir_form_on_the_rule_s_edges():
    one = np.ones(1, np.float32)
    # first order: the 1e-12 rule is accepted for 1 .. 128 chunks; p^16 == 0 counts as one chunk; |p| = 1 never decays
    assert F.iir_form(one, [1, 0.0])[0::4] == ("oneshot", 1) and F.iir_form(one, [1, 0.0])[5] == 1
    assert F.iir_form(one, [1, -0.5])[5] == 3                   # ceil(log 1e-12 / log 0.5^16) = ceil(2.49)
    assert F.iir_form(one, [1, -1.0])[0] == "threepass" and F.iir_form(one, [1, 1.0])[0] == "threepass"
    # a[0] only scales: the normalised taps decide
    assert F.iir_form(2 * one, [2, -2.0])[0] == "threepass" and F.iir_form(one, [4, -2.0]) == F.iir_form(one, [1, -0.5])
    # NBT and the compile-time tap counts
    b, a = F.placed_filter(4, 0.85, 8, 1)
    assert [F.iir_form(b[:k], a)[2:4] for k in (1, 2, 3, 4, 5, 6, 7, 8)] == [(2, "NBT-1"), (2, "NBT"), (4, "NBT-1"), (4, "NBT"), (8, "NBT-3"), (8, "NBT-2"),
                                                                             (8, "NBT-1"), (8, "NBT")]
    b, a = F.placed_filter(5, 0.85, 16, 1)
    assert [F.iir_form(b[:k], a)[2:4] for k in (5, 8, 14, 15, 16)] == [(16, "predicated")] * 3 + [(16, "NBT-1"), (16, "NBT")]
    # the scan path's limits
    assert F.iir_form(np.ones(17, np.float32), a)[0] == "seq" and F.iir_form(one, np.ones(10, np.float32))[0] == "seq" and F.iir_form(one, one)[0] == "seq"


GROUPS = {"cross": F.form_cross_cases, "sweep": F.tap_sweep_cases, "seq": F.seq_cases, "carry": F.carry_cases, "run2": lambda: F.run2_cases(256),
          "misaligned": F.misaligned_cases}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_case_is_well_conditioned(group):
    """a condition on the table, not a measurement of the library: sequential Float32 against f64 on the case's own input"""
    bad, worst = [], (0.0, None)
    for c in GROUPS[group]():
        x, want, yard, scale = F.reference(c)
        assert np.all(np.isfinite(want.view(np.float32))), c.name
        rel = yard / F.conditioning_limit(c, scale)
        worst = max(worst, (rel, c.name))
        if rel > 1.0:
            bad.append("%s: yard %.3g, scale %.3g, limit %.3g" % (c.name, yard, scale, F.conditioning_limit(c, scale)))
    print("%s: worst yard / limit %.3g (%s)" % (group, worst[0], worst[1]))
    assert not bad, "\n".join(bad)
