"""The guard checks of tests/helpers/guarded.py on numpy arrays: a clean fake kernel passes, and each planted fault - a word written before the
output, a word written after the count, a hole inside [0, count), a modified input byte, an output that depends on an input guard word - is
reported with its position.  This is what shows that tests/test_gpu_bounds.py can fail; no wrong kernel is built or run on a GPU for it."""
import numpy as np
import pytest

from tests.helpers import guarded as GD

LENS = [1027, 515]


def f32(h, off, n):
    return np.frombuffer(h[off:off + 4 * n].tobytes(), "<f4")


def put(h, off, values):
    raw = np.frombuffer(np.asarray(values, "<f4").tobytes(), np.uint8)
    h[off:off + len(raw)] = raw


class Fake:
    """y[i] = 2 x[i] + (the last sample of the previous call), one output per input; `fault` plants one defect"""

    def __init__(self, fault=None, counted=False):
        self.fault, self.counted, self.carry = fault, counted, np.float32(0)

    def max_output(self, n):
        return n

    def __call__(self, ins, n, outs, cap):
        (xh, xo), (yh, yo) = ins[0], outs[0]
        x = f32(xh, xo, n)
        count = n - n // 3 if self.counted else n          # a counted stage: fewer outputs than the capacity
        y = (2 * x + self.carry)[:count].astype("<f4")
        self.carry = x[-1]
        if self.fault == "guard-dependent":
            after = np.frombuffer(xh[xo + 4 * n:xo + 4 * n + 4].tobytes(), "<u4")[0]      # the word behind the input
            y[-1] += np.float32((int(after) >> 30) & 1)
        put(yh, yo, y)
        if self.fault == "before":
            put(yh, yo - 4, [1.5])
        if self.fault == "far-before":
            put(yh, yo - 4 * GD.G_WORDS, [1.5])
        if self.fault == "after":
            put(yh, yo + 4 * count, [1.5])
        if self.fault == "up-to-capacity" and count < cap:
            put(yh, yo + 4 * (cap - 1), [0.0])
        if self.fault == "hole" and count > 700:
            yh[yo + 4 * 700:yo + 4 * 701] = np.roll(GD.SENT_BYTES, -(yo % 4))          # as the fill left it
        if self.fault == "nan" and count > 5:
            put(yh, yo + 20, [np.inf])
        if self.fault == "input":
            xh[xo + 4 * n + 9] ^= 1
        return count


def run(fault=None, counted=False, in_off=0, out_off=0, check=None):
    x = np.random.default_rng(3).uniform(-1, 1, sum(LENS)).astype(np.float32)
    return GD.run_guarded(lambda: Fake(fault, counted), [x], LENS, in_off, out_off, mem=GD.NumpyMemory(),
                          call=lambda obj, ins, n, outs, cap: obj(ins, n, outs, cap), max_output=lambda obj, n: obj.max_output(n), check=check), x


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (0, 1), (3, 3)])
@pytest.mark.parametrize("counted", [False, True])
def test_clean_fake_passes(in_off, out_off, counted):
    seen = []
    got, x = run(None, counted, in_off, out_off, check=lambda c, y: seen.append(c))
    assert seen == [0, 1] and [len(g) for g in got] == [n - n // 3 if counted else n for n in LENS]
    assert np.array_equal(got[0], (2 * x[:LENS[0]])[:len(got[0])])
    assert np.array_equal(got[1], (2 * x[LENS[0]:] + x[LENS[0] - 1])[:len(got[1])])             # state crossed the call boundary


@pytest.mark.parametrize("fault,counted,report", [
    ("before", False, r"\(a\) write before out0: word -1 "),
    ("far-before", False, r"\(a\) write before out0: word -4096 "),
    ("after", False, r"\(b\) write at or after the count of 4108 bytes of out0: word 1027 "),
    ("after", True, r"\(b\) write at or after the count of 2740 bytes of out0: word 685 "),
    ("up-to-capacity", True, r"\(b\) write at or after the count .* word 1026 "),
    ("hole", False, r"\(c\) unwritten sample 700 of out0: word 700 "),
    ("nan", False, r"\(c\) non-finite float 5 of out0"),
    ("input", False, r"\(d\) in0 modified: word 1029 \(byte 4117\)"),
    ("guard-dependent", False, r"\(e\) call 0 depends on bytes outside its input: first differing output word 1026 "),
])
@pytest.mark.parametrize("off", [0, 1])
def test_each_planted_fault_is_reported(fault, counted, report, off):
    with pytest.raises(GD.GuardViolation, match=report):
        run(fault, counted, off, off)


def test_oracle_failure_reaches_the_caller():
    """(f): a tail that is in bounds and wrong does not pass"""
    def check(c, y):
        assert y[-1] == 0, "call %d tail" % c
    with pytest.raises(AssertionError, match="call 0 tail"):
        run(None, check=check)


def test_byte_streams_and_byte_offsets():
    """one-byte samples at an odd byte offset: the guards are checked to the byte, the fills are 0xFF and 0x00"""
    bits = np.random.default_rng(4).integers(0, 2, 700).astype(np.uint8)
    fills = set()

    def call(obj, ins, n, outs, cap, bad=None):
        (xh, xo), (yh, yo) = ins[0], outs[0]
        fills.add(int(xh[xo - 1]))
        yh[yo:yo + n] = xh[xo:xo + n] ^ 1
        if bad is not None:
            yh[yo + bad] = 7
        return n

    kw = dict(mem=GD.NumpyMemory(), max_output=lambda obj, n: n, in_kind="bits", out_dtype=np.uint8, offsets_in_bytes=True)
    got = GD.run_guarded(lambda: None, [bits], [401, 299], 1, 3, call=call, **kw)
    assert fills == {0xFF, 0x00} and np.array_equal(np.concatenate(got), bits ^ 1)
    with pytest.raises(GD.GuardViolation, match=r"\(b\) .* \(byte 401\)"):
        GD.run_guarded(lambda: None, [bits], [401, 299], 1, 3, call=lambda *a: call(*a, bad=401), **kw)
    with pytest.raises(GD.GuardViolation, match=r"\(a\) .* \(byte -1\)"):
        GD.run_guarded(lambda: None, [bits], [401, 299], 1, 3, call=lambda *a: call(*a, bad=-1), **kw)
