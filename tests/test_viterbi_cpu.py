"""ConvolutionalEncoderBlock and ViterbiDecoderBlock without a device: the encoder's convention, the model of tests/helpers/viterbi_model.py on
noise-free and noisy streams (windowed against full-sequence, array form against the literal loop), the count arithmetic of
luaradio_amd/csrc/viterbi_plan.h (tools/host_viterbi_check.hip, built for the host) against Python's integers, and the refusals of the blocks'
arguments and of the op strings, which need no device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests.helpers import viterbi_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K7 = (7, [0o171, 0o133])


def test_encoder_convention():
    """K = 7, (171, 133), a one and six zeros: the polynomials read from bit 6 down"""
    out = vm.encode(7, [0o171, 0o133], [1, 0, 0, 0, 0, 0, 0])
    assert out.reshape(-1, 2).tolist() == [[1, 1], [1, 0], [1, 1], [1, 1], [0, 0], [0, 1], [1, 1]]
    assert [list(map(int, "%d%d" % tuple(p))) for p in out.reshape(-1, 2)] == [[1, 1], [1, 0], [1, 1], [1, 1], [0, 0], [0, 1], [1, 1]]
    # the state is r >> 1: a stream cut anywhere continues
    enc = vm.EncoderModel(7, [0o171, 0o133])
    msg = np.random.default_rng(0).integers(0, 2, 50)
    assert np.array_equal(np.concatenate([enc.process(msg[:13]), enc.process(msg[13:])]), vm.encode(7, [0o171, 0o133], msg))


@pytest.mark.parametrize("K,polys", [(3, [0o7, 0o5]), K7, (9, [0o561, 0o753]), (7, [0o133, 0o171, 0o165])], ids=["k3", "k7", "k9", "k7-third"])
def test_noise_free_round_trip_is_exact(K, polys):
    """a wrong start state falls strictly behind within K - 1 steps, so with q = +-127 the true path is the unique maximum: D = 64, L = K - 1"""
    D, L = 64, K - 1
    msg = np.random.default_rng(K).integers(0, 2, 6 * D + L + 9).astype(np.uint8)
    code = vm.encode(K, polys, msg)
    for q in (vm.quantise_bits(code), vm.quantise(100.0 * (1.0 - 2.0 * code), 8.0)):
        assert set(np.unique(q)) == {-127, 127}
        out = vm.decode_windows(K, polys, q, D, L)
        assert len(out) == 6 * D and np.array_equal(out, msg[:len(out)])
    # the streaming form, cut into calls
    model = vm.DecoderModel(K, polys, False, 8.0, D, L)
    parts = [model.process(code[a:b]) for a, b in zip([0, 1, 100, 100, 517], [1, 100, 100, 517, len(code)])]
    assert np.array_equal(np.concatenate(parts), msg[:6 * D]) and len(parts[0]) == 0


AWGN = [(2.0, 1), (2.0, 3), (3.0, 1), (3.0, 2)]
_STREAMS = {}


def awgn_stream(ebn0_db, seed, nbits=63 * 256):
    """K = 7, rate 1/2, scale 8: (the message, the quantised inputs of nbits + 48 steps)"""
    if (ebn0_db, seed) not in _STREAMS:
        rng = np.random.default_rng(seed)
        msg = rng.integers(0, 2, nbits + 48).astype(np.uint8)
        q = vm.quantise(vm.awgn_llrs(rng, vm.encode(*K7, msg), ebn0_db, 0.5), 8.0)
        q.setflags(write=False)
        _STREAMS[(ebn0_db, seed)] = (msg, q)
    return _STREAMS[(ebn0_db, seed)]


@pytest.mark.parametrize("ebn0_db,seed", AWGN)
def test_windowed_against_full_sequence(ebn0_db, seed):
    """D = 256, L = 8 (K - 1) = 48: at most 1 disagreement per 4096 decoded bits with one window over the whole stream.  Found with these seeds:
    0 disagreements over 16 128 bits in all four streams (106 and 102 message errors at 2 dB, 13 and 6 at 3 dB, the same for both decoders); at
    L = 24 the decoders disagree on 1, 0, 1 and 0 bits, which is printed and not held to a cap."""
    msg, q = awgn_stream(ebn0_db, seed)
    full = vm.decode_full(*K7, q)
    for L, cap in ((48, 16128 // 4096), (24, None)):
        out = vm.decode_windows(*K7, q, 256, L)
        assert len(out) == 16128
        differ = int(np.count_nonzero(out != full[:len(out)]))
        print("Eb/N0 %.0f dB seed %d L %d: %d disagreements, %d / %d message errors (windowed / full)"
              % (ebn0_db, seed, L, differ, np.count_nonzero(out != msg[:len(out)]), np.count_nonzero(full[:len(out)] != msg[:len(out)])))
        assert cap is None or differ <= cap, (L, differ)


@pytest.mark.parametrize("ebn0_db,seed", AWGN)
def test_array_form_equals_the_literal_loop(ebn0_db, seed):
    """bit for bit on all 63 windows of those streams"""
    _, q = awgn_stream(ebn0_db, seed)
    a, b = vm.decode_windows(*K7, q, 256, 48), vm.decode_windows(*K7, q, 256, 48, literal=True)
    assert len(a) == 63 * 256 and np.array_equal(a, b)


@pytest.mark.parametrize("K,polys", [(3, [0o7, 0o5]), (9, [0o561, 0o753]), (7, [0o133, 0o171, 0o165]), (8, [0o247, 0o371])], ids=["k3", "k9", "k7-third", "k8"])
def test_array_form_equals_the_literal_loop_on_ties(K, polys):
    """inputs from {-1, 0, 1}, where almost every comparison ties, through the streaming model cut into calls"""
    rng = np.random.default_rng(K)
    n, D, L = len(polys), 64, 2 * (K - 1)
    x = (rng.integers(-1, 2, n * (2 * D + L + 3)) / 8.0).astype(np.float32)
    a, b = vm.DecoderModel(K, polys, True, 8.0, D, L), vm.DecoderModel(K, polys, True, 8.0, D, L, literal=True)
    cuts = [0, 5, n * (D + L) - 1, n * (D + L), len(x)]
    got = [(a.process(x[i:j]), b.process(x[i:j])) for i, j in zip(cuts[:-1], cuts[1:])]
    assert [len(g[0]) for g in got] == [0, 0, D, D] and all(np.array_equal(u, v) for u, v in got)


# ---- viterbi_plan.h against Python integers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/host_viterbi_check.hip as plain C++; returns ask(lines) -> the answers, one list of integers per line"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("vitcheck")
    exe = str(d / "host_viterbi_check")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tools", "host_viterbi_check.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    def ask(lines):
        listing = str(d / "cases.txt")
        with open(listing, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, listing], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = r.stdout.strip().split("\n")
        assert len(out) == len(lines) and all(o.split()[0] == ln.split()[0] for o, ln in zip(out, lines))
        return [[int(v) for v in o.split()[1:]] for o in out]
    return ask


SHAPES = [(2, 64, 24), (3, 64, 6), (2, 512, 48), (4, 2048, 256), (2, 100, 7)]


@pytest.mark.parametrize("n,D,L", SHAPES)
def test_emitted_bits_for_every_cut_of_a_short_stream(checker, n, D, L):
    total = n * (3 * D + L) + 5
    if D > 512:
        ends = sorted({0, 1, n * L, n * (D + L) - 1, n * (D + L), n * (D + L) + 1, n * (2 * D + L) - 1, n * (2 * D + L), total})
    else:
        ends = list(range(total + 1))
    got = checker(["done %d %d %d %d" % (n, D, L, q) for q in ends])
    for q, (windows, bits) in zip(ends, got):
        assert windows == vm.windows_done(q, n, D, L) and bits == windows * D, q
    assert got[-1][0] == 3
    # a window leaves with the input that completes its last step, and every call's count stays inside max_output
    done = {q: w for q, (w, _) in zip(ends, got)}
    for w in (1, 2):
        assert done[n * (w * D + L) - 1] == w - 1 and done[n * (w * D + L)] == w
    for a in ends[::max(1, len(ends) // 9)]:
        sizes = sorted({e - a for e in ends if e >= a})
        bounds = [b for (b,) in checker(["max %d %d %d %d" % (n, D, L, s) for s in sizes])]
        for s, bound in zip(sizes, bounds):
            assert bound == vm.max_output(s, n, D, L) and (done[a + s] - done[a]) * D <= bound, (a, s)


def test_max_output_is_never_below_the_true_count(checker):
    """and is reached: a call of one input can complete a window"""
    n, D, L = 3, 64, 10
    assert checker(["max %d %d %d 0" % (n, D, L), "max %d %d %d 1" % (n, D, L), "max %d %d %d %d" % (n, D, L, n * D), "max %d %d %d %d" % (n, D, L, n * D + 1)]) \
        == [[0], [D], [D], [2 * D]]
    assert vm.windows_done(n * (D + L), n, D, L) - vm.windows_done(n * (D + L) - 1, n, D, L) == 1
    assert vm.windows_done(n * (2 * D + L), n, D, L) - vm.windows_done(n * (D + L) - 1, n, D, L) == 2      # n D + 1 inputs, two windows
    rng = np.random.default_rng(5)
    for _ in range(2000):
        q, size = int(rng.integers(0, 4000)), int(rng.integers(0, 1500))
        assert vm.bits_done(q + size, n, D, L) - vm.bits_done(q, n, D, L) <= vm.max_output(size, n, D, L)


@pytest.mark.parametrize("n,D,L", SHAPES)
def test_counts_near_2_to_the_64(checker, n, D, L):
    top = (1 << 64) - 1
    qs = [top, top - 1, top - n, (1 << 63) + 12345, (1 << 40) + 3, (1 << 40) + n * D + 1, n * L - 1, n * L, 0]
    for q, (windows, bits) in zip(qs, checker(["done %d %d %d %d" % (n, D, L, q) for q in qs])):
        assert windows == vm.windows_done(q, n, D, L) and bits == vm.bits_done(q, n, D, L) < (1 << 64), q
    ws = [0, 1, 2, vm.windows_done(top, n, D, L) - 1, vm.windows_done(top, n, D, L)]
    for w, (t0, t1, steps) in zip(ws, checker(["win %d %d %d %d" % (n, D, L, w) for w in ws])):
        assert (t0, t1, steps) == (vm.first_step(w, D, L), vm.last_step(w, D, L), vm.last_step(w, D, L) - vm.first_step(w, D, L) + 1) and steps <= D + 2 * L
    for w, (base,) in zip(ws, checker(["base %d %d %d %d" % (n, D, L, w) for w in ws])):
        assert base == n * vm.first_step(w, D, L) < (1 << 64)
    assert checker(["max %d %d %d %d" % (n, D, L, top)]) == [[min(vm.max_output(top, n, D, L), top)]]
    assert checker(["shape %d %d %d" % (n, D, L)]) == [[vm.memory(n, D, L), n * (D + 2 * L + 1)]]


@pytest.mark.parametrize("n,D,L", SHAPES)
def test_seek_anywhere_and_what_is_carried(checker, n, D, L):
    """a seek to n0, also with n0 mod n != 0, lands on the bits emitted by then, and the inputs carried from the first step of the next window on
    fit the carry buffer"""
    n0s = [0, 1, n - 1, n, n * L + 1, n * (D + L) - 1, n * (D + L), n * (D + L) + 1, n * (5 * D + L) + n - 1, (1 << 40) + 3, (1 << 40) + n * D + 1]
    got = checker(["done %d %d %d %d" % (n, D, L, q) for q in n0s])
    bases = checker(["base %d %d %d %d" % (n, D, L, w) for w, _ in got])
    for n0, (w, bits), (base,) in zip(n0s, got, bases):
        assert bits == vm.bits_done(n0, n, D, L) and base <= n0 and n0 - base < n * (D + 2 * L + 1), n0
    # memory(): the window that input i completes reads nothing in front of n0 once i >= n0 + memory, and one input less is not enough
    M = vm.memory(n, D, L)
    for w in (1, 2, 7):
        completes, first_input = n * (w * D + D + L) - 1, n * (w * D - L)
        if first_input > 0:
            assert completes - M == first_input and completes - (M - 1) > first_input


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------------------
CODE_REFUSALS = [((2, [3, 1]), "constraint length must be 3 .. 9 (got 2)"), ((10, [0o1001, 0o1777]), "constraint length must be 3 .. 9 (got 10)"),
                 ((7, [0o171]), "the number of polynomials must be 2 .. 4 (got 1)"), ((7, [0o171, 0o133, 0o165, 0o117, 0o155]), "must be 2 .. 4 (got 5)"),
                 ((7, [0o171, 0o333]), "polynomial 333 (octal) has bits at or above the constraint length 7"),
                 ((7, [0o71, 0o33]), "no polynomial of 71,33 has bit 6 set"), ((7, [0o170, 0o132]), "no polynomial of 170,132 has bit 0 set")]
CODE_IDS = ["k 2", "k 10", "one polynomial", "five polynomials", "polynomial too wide", "no bit k - 1", "no bit 0"]


@pytest.mark.parametrize("cls,who", [(lr.ConvolutionalEncoderBlock, "convenc"), (lr.ViterbiDecoderBlock, "viterbi")])
@pytest.mark.parametrize("args, fragment", CODE_REFUSALS, ids=CODE_IDS)
def test_defective_codes_are_refused(cls, who, args, fragment):
    with pytest.raises(ValueError) as e:
        cls(*args)
    assert str(e.value).startswith(who + ":") and fragment in str(e.value), str(e.value)
    # and by the library, in front of the device, with the same words
    K, polys = args
    op = "%s:k=%d:polys=%s" % (who, K, ",".join("%o" % g for g in polys)) + (":input=llr:scale=8:block=512:depth=48" if who == "viterbi" else "")
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith(who + ":") and fragment in message, message


OPTION_REFUSALS = [({"scale": 0.0}, "scale must be a finite Float32 above 0 (got 0"), ({"scale": float("nan")}, "scale must be a finite Float32 above 0 (got nan"),
                   ({"scale": float("inf")}, "scale must be a finite Float32 above 0 (got inf"), ({"scale": -1.0}, "scale must be a finite Float32 above 0 (got -1"),
                   ({"block": 63}, "block must be 64 .. 2048 decoded bits (got 63)"), ({"block": 2049}, "block must be 64 .. 2048 decoded bits (got 2049)"),
                   ({"depth": 5}, "depth must be 6 .. 256 steps (got 5)"), ({"depth": 257}, "depth must be 6 .. 256 steps (got 257)")]


@pytest.mark.parametrize("options, fragment", OPTION_REFUSALS, ids=[f for _, f in OPTION_REFUSALS])
def test_defective_options_are_refused(options, fragment):
    with pytest.raises(ValueError) as e:
        lr.ViterbiDecoderBlock(*K7, options)
    assert str(e.value).startswith("viterbi:") and fragment in str(e.value), str(e.value)
    fields = {"scale": "8", "block": "512", "depth": "48"}
    fields.update({k: repr(v) if isinstance(v, float) else str(v) for k, v in options.items()})
    op = "viterbi:k=7:polys=171,133:input=llr:scale=%(scale)s:block=%(block)s:depth=%(depth)s" % fields
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith("viterbi:") and fragment in message, message


def test_decision_words_beyond_64_kib_are_refused():
    """(D + 2 L) 2^(K - 1) / 8: K = 9 takes 32 bytes per step, so 2048 steps are the most"""
    assert lr.ViterbiDecoderBlock(9, [0o561, 0o753], {"block": 1024, "depth": 256}).block == 1024
    assert lr.ViterbiDecoderBlock(9, [0o561, 0o753], {"block": 1952, "depth": 48}).depth == 48            # 2048 steps: 65 536 bytes
    assert lr.ViterbiDecoderBlock(8, [0o247, 0o371], {"block": 2048, "depth": 256}).depth == 256           # 2560 steps of 16 bytes
    with pytest.raises(ValueError) as e:
        lr.ViterbiDecoderBlock(9, [0o561, 0o753], {"block": 1953, "depth": 48})
    assert "= 65568 bytes, exceed 65536" in str(e.value)
    L = _lib.load()
    assert not L.lrhip_unary_create(b"viterbi:k=9:polys=561,753:input=llr:scale=8:block=2048:depth=64", 0.0, 0.0, 0, 0)
    assert "= 69632 bytes, exceed 65536" in L.lrhip_strerror().decode()


OP_REFUSALS = [("convenc:k=7:polys=171,133:bogus=1", "unknown parameter \"bogus\""), ("convenc:k=7", "missing parameter \"polys\""),
               ("convenc:polys=171,133", "missing parameter \"k\""), ("convenc:k=7:polys=171,138", "bad polynomial 1 \"138\" (octal digits)"),
               ("convenc:k=7:polys=171,", "bad polynomial 1 \"\""), ("convenc:k=seven:polys=171,133", "bad value for \"k\""),
               ("viterbi:k=7:polys=171,133:input=f16:scale=8:block=512:depth=48", "unsupported input \"f16\""),
               ("viterbi:k=7:polys=171,133:input=llr:block=512:depth=48", "missing parameter \"scale\""),
               ("viterbi:k=7:polys=171,133:input=llr:scale=8:block=512", "missing parameter \"depth\""),
               ("viterbi:k=7:polys=171,133:input=llr:scale=8:block=5e2:depth=48", "bad value for \"block\"")]


@pytest.mark.parametrize("op, fragment", OP_REFUSALS, ids=[f for _, f in OP_REFUSALS])
def test_defective_op_strings_are_refused_in_front_of_the_device(op, fragment):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith(op.split(":")[0] + ":") and fragment in message, message


def test_op_strings_of_the_blocks():
    """what the blocks hand to lrhip_unary_create: octal polynomials, every option spelled out; the library has no complaint about the text (without a
    device its only refusal is the missing device)"""
    enc = lr.ConvolutionalEncoderBlock(7, [0o171, 0o133])
    assert enc.op() == "convenc:k=7:polys=171,133"
    dec = lr.ViterbiDecoderBlock(7, (0o171, 0o133))
    assert (dec.soft, float(dec.scale), dec.block, dec.depth) == (True, 8.0, 512, 48) and dec.memory() == 2 * (512 + 96) - 1
    assert dec.op() == "viterbi:k=7:polys=171,133:input=llr:scale=8:block=512:depth=48"
    third = lr.ViterbiDecoderBlock(9, np.array([0o557, 0o663, 0o711]), {"soft": False, "scale": 0.1, "block": 64, "depth": 8})
    assert third.op() == "viterbi:k=9:polys=557,663,711:input=bit:scale=0.100000001:block=64:depth=8"
    enc.rate = 1200.0
    dec.rate = 2400.0
    assert enc.get_rate() == 2400.0 and dec.get_rate() == 1200.0
    for blk, in_type, out_type in ((enc, types.Bit, types.Bit), (dec, types.Float32, types.Bit), (third, types.Bit, types.Bit)):
        blk.differentiate([in_type])
        assert blk.get_output_type() is out_type
        L = _lib.load()
        ptr = L.lrhip_unary_create(blk.op().encode(), 0.0, 0.0, 0, 0)
        if ptr:
            L.lrhip_stage_destroy(ptr)
        else:
            assert not L.lrhip_strerror().decode().startswith(blk.op().split(":")[0] + ":"), L.lrhip_strerror().decode()
    with pytest.raises(TypeError):
        dec.differentiate([types.Bit])


@pytest.mark.parametrize("args, fragment", [((True, [0o7, 0o5]), "constraint length must be 3 .. 9 (got True)"),
                                            ((7, [121.0, 91.0]), "polynomials must be integers (got 121.0)"),
                                            ((7, [0o171, True]), "polynomials must be integers (got True)"),
                                            ((7, [0o171, 0o133], {"block": True}), "block must be 64 .. 2048 decoded bits (got True)"),
                                            ((7, [0o171, 0o133], {"block": 512.0}), "block must be 64 .. 2048 decoded bits (got 512.0)"),
                                            ((7, [0o171, 0o133], {"depth": True}), "depth must be 6 .. 256 steps (got True)")],
                         ids=["k bool", "float polynomials", "bool polynomial", "block bool", "block float", "depth bool"])
def test_arguments_of_the_wrong_kind_are_refused(args, fragment):
    """a bool is no count and a float is no polynomial: nothing is truncated or taken for 1"""
    for cls in (lr.ViterbiDecoderBlock,) if len(args) == 3 else (lr.ViterbiDecoderBlock, lr.ConvolutionalEncoderBlock):
        with pytest.raises(ValueError) as e:
            cls(*args)
        assert fragment in str(e.value), str(e.value)
