"""ReedSolomonEncoderBlock, ReedSolomonDecoderBlock, PackBitsBlock and UnpackBitsBlock without a device.  The model of
tests/helpers/reedsolomon_model.py is the contract, so it is held to properties that do not use its own tables - a second GF(2^8) multiply, carry-less
shift-and-reduce, does the evaluations here -: codewords vanish at the roots, up to t errors are corrected, a decode of more is either flagged or a
codeword within t of the received word, and a flagged word has no codeword within t (by enumeration in two small codes).  Then the header
luaradio_amd/csrc/rs_plan.h (tools/host_rs_check.hip, built for the host) against Python's integers and the model, and the refusals of the blocks'
arguments and of the op strings, which need no device."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests.helpers import reedsolomon_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = rm.PARAMETER_SETS


# ---- a second arithmetic ----------------------------------------------------------------------------------------------------------------------------
def clmul(a, b, gfpoly):
    """a b in GF(2)[x] / gfpoly, bit by bit"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x100:
            a ^= gfpoly
    return r


_TABLES = {}


def product_table(gfpoly):
    """[a][b] -> a b, from clmul alone"""
    if gfpoly not in _TABLES:
        table = np.array([[clmul(a, b, gfpoly) for b in range(256)] for a in range(256)], np.uint8)
        table.setflags(write=False)
        _TABLES[gfpoly] = table
    return _TABLES[gfpoly]


def root_values(n, k, gfpoly=0x11d, fcr=0, prim=1):
    """alpha^((fcr + i) prim) by repeated multiplication with 2"""
    out = []
    for i in range(n - k):
        x = 1
        for _ in range(((fcr + i) * prim) % 255):
            x = clmul(x, 2, gfpoly)
        out.append(x)
    return out


def syndromes(word, n, k, gfpoly=0x11d, fcr=0, prim=1):
    """the word, byte j the coefficient of x^(n - 1 - j), at every root: Horner with the product table"""
    table = product_table(gfpoly)
    out = []
    for root in root_values(n, k, gfpoly, fcr, prim):
        y = 0
        for v in word:
            y = int(table[y, root]) ^ int(v)
        out.append(y)
    return out


def corrupt(rng, word, count):
    out = list(word)
    for p in rng.choice(len(word), count, replace=False):
        out[p] ^= int(rng.integers(1, 256))
    return out


def distance(a, b):
    return sum(int(u) != int(v) for u, v in zip(a, b))


# ---- the model against properties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_codewords_vanish_at_every_root(name):
    n, k, kw = SETS[name]
    code = rm.Code(n, k, **kw)
    rng = np.random.default_rng(n + k)
    for message in (rng.integers(0, 256, k), np.full(k, 255), np.eye(1, k, k - 1, dtype=np.int64)[0], np.eye(1, k, 0, dtype=np.int64)[0]):
        word = code.encode(message)
        assert word[:k] == [int(v) for v in message] and len(word) == n
        assert syndromes(word, n, k, **kw) == [0] * (n - k)
    assert code.generator[-1] == 1 and len(code.generator) == n - k + 1
    assert code.roots == root_values(n, k, **kw)


@pytest.mark.parametrize("name", list(SETS))
def test_up_to_t_errors_are_corrected(name):
    n, k, kw = SETS[name]
    code = rm.Code(n, k, **kw)
    t = code.t
    rng = np.random.default_rng(n * k)
    message = [int(v) for v in rng.integers(0, 256, k)]
    word = code.encode(message)
    for count in sorted({0, 1, 2, t // 2, t - 1, t} & set(range(t + 1))):
        for _ in range(3):
            assert code.decode(corrupt(rng, word, count)) == (message, count), (name, count)
    # parity only, both ends, a burst, both extreme magnitudes
    ends = list(word)
    ends[0] ^= 0x01
    if t >= 2:
        ends[n - 1] ^= 0xFF
    assert code.decode(ends) == (message, min(t, 2))
    parity_only = list(word)
    for p in range(k, k + t):
        parity_only[p] ^= 0xFF
    assert code.decode(parity_only) == (message, t)
    burst = list(word)
    for p in range(k // 2, k // 2 + t):
        burst[p] ^= int(rng.integers(1, 256))
    assert code.decode(burst) == (message, t)


@pytest.mark.parametrize("name", list(SETS))
def test_beyond_t_is_flagged_or_a_legitimate_miscorrection(name):
    n, k, kw = SETS[name]
    code = rm.Code(n, k, **kw)
    t = code.t
    rng = np.random.default_rng(n ^ k)
    word = code.encode(rng.integers(0, 256, k))
    outcomes = set()
    for count in [t + 1] * 8 + [t + 2] * 4 + [min(n, 2 * t + 1)] * 2 + [n] * 2:
        received = corrupt(rng, word, min(count, n))
        out, status = code.decode(received)
        if status == rm.UNCORRECTABLE:
            assert out == received[:k]
        else:
            again = code.encode(out)
            assert 0 <= status <= t and distance(again, received) == status and syndromes(again, n, k, **kw) == [0] * (n - k)
        outcomes.add(status == rm.UNCORRECTABLE)
    assert True in outcomes or t == 1


def within_t_syndromes(n, k):
    """the packed syndromes of EVERY error pattern of weight 1 .. t, t = (n - k) / 2 <= 2, from the product table: S_i(e) = sum e_p root_i^p"""
    table, t = product_table(0x11d), (n - k) // 2
    powers = np.ones((n - k, n), np.uint8)                          # [i][p] = root_i^p
    for i, root in enumerate(root_values(n, k)):
        for p in range(1, n):
            powers[i, p] = table[powers[i, p - 1], root]
    values = np.arange(1, 256)
    single = np.stack([table[values[:, None], powers[i][None, :]] for i in range(n - k)]).astype(np.uint32)      # [i][value][p]
    packed = sum(single[i] << (8 * i) for i in range(n - k))                                                    # [value][p]
    found = [packed.ravel()]
    if t == 2:
        for a, b in itertools.combinations(range(n), 2):
            found.append((packed[:, a][:, None] ^ packed[:, b][None, :]).ravel())
    return np.unique(np.concatenate(found))


@pytest.mark.parametrize("n,k,count", [(10, 8, 10 * 255), (12, 8, 12 * 255 + 66 * 255 * 255)], ids=["10-8", "12-8"])
def test_a_flagged_word_has_no_codeword_within_t(n, k, count):
    """completeness: all words within distance t of a flagged word, 10 * 255 of them in (10, 8) and C(12, 2) * 255^2 = 4.3 M (and 12 * 255) in
    (12, 8), have a non-zero syndrome - that is, the syndromes of the flagged word are those of no error pattern of weight <= t"""
    code = rm.Code(n, k)
    t = code.t
    reachable = within_t_syndromes(n, k)
    table = product_table(0x11d)
    # (every pattern has its own syndromes: t errors are correctable; so the enumeration is complete when the count is right)
    assert len(reachable) == count
    rng = np.random.default_rng(n)
    word = code.encode(rng.integers(0, 256, k))
    flagged = 0
    for _ in range(600):
        received = corrupt(rng, word, int(rng.integers(t + 1, n + 1)))
        out, status = code.decode(received)
        S = syndromes(received, n, k)
        key = sum(s << (8 * i) for i, s in enumerate(S))
        if status == rm.UNCORRECTABLE:
            flagged += 1
            assert key != 0 and key not in reachable[np.searchsorted(reachable, key):][:1]
        else:
            assert key in reachable[np.searchsorted(reachable, key):][:1] and 1 <= status <= t
    assert flagged >= 300 and table[2, 2] == 4


def test_both_outcomes_of_two_errors_in_10_8():
    """512 words of (10, 8) with two errors: the share that lands within distance 1 of another codeword is about n 255 / 65535 = 3.9 %; at least 8 of
    each outcome, so neither path can be left out"""
    code = rm.Code(10, 8)
    rng = np.random.default_rng(2024)
    flagged = miscorrected = 0
    for _ in range(512):
        message = [int(v) for v in rng.integers(0, 256, 8)]
        received = corrupt(rng, code.encode(message), 2)
        out, status = code.decode(received)
        if status == rm.UNCORRECTABLE:
            flagged += 1
            assert out == received[:8]
        else:
            miscorrected += 1
            assert status == 1 and distance(code.encode(out), received) == 1 and out != message
    print("(10, 8), two errors: %d flagged, %d miscorrected" % (flagged, miscorrected))
    assert flagged >= 8 and miscorrected >= 8 and flagged + miscorrected == 512


def test_ccsds_with_17_errors():
    n, k, kw = SETS["ccsds"]
    code = rm.Code(n, k, **kw)
    rng = np.random.default_rng(17)
    word = code.encode(rng.integers(0, 256, k))
    flagged = 0
    for _ in range(40):
        received = corrupt(rng, word, 17)
        out, status = code.decode(received)
        if status == rm.UNCORRECTABLE:
            flagged += 1
            assert out == received[:k]
        else:
            assert distance(code.encode(out), received) == status <= 16
    print("CCSDS (255, 223), 17 errors: %d of 40 flagged" % flagged)
    assert flagged >= 30


def test_frames_interleave_and_streaming():
    n, k, kw = SETS["ccsds"]
    code, I = rm.Code(n, k, **kw), 3
    rng = np.random.default_rng(5)
    message = rng.integers(0, 256, 2 * I * k + 7).astype(np.uint8)
    enc = rm.encoder_model(n, k, interleave=I, **kw)
    parts = [enc.process(message[a:b]) for a, b in zip([0, 1, I * k - 1, I * k, I * k], [1, I * k - 1, I * k, I * k, len(message)])]
    assert [len(p) for p in parts] == [0, 0, I * n, 0, I * n]
    sent = np.concatenate(parts)
    for f in range(2):
        frame = sent[f * I * n:(f + 1) * I * n]
        assert np.array_equal(frame[:I * k], message[f * I * k:(f + 1) * I * k])
        for c in range(I):
            assert syndromes(frame[c::I], n, k, **kw) == [0] * (n - k)
    # a burst of I t bytes anywhere in a frame is t errors per codeword
    received = sent.copy()
    received[100:100 + I * code.t] ^= 0x5A
    dec = rm.decoder_model(n, k, interleave=I, status=True, **kw)
    out = dec.process(received)
    assert np.array_equal(out[:I * k], message[:I * k]) and out[I * k:I * k + I].tolist() == [code.t] * I and out[-I:].tolist() == [0] * I
    assert dec.memory() == I * n - 1 and enc.memory() == I * k - 1 and dec.max_output(1) == I * (k + 1) and dec.max_output(I * n + 1) == 2 * I * (k + 1)
    # a seek into a frame counts the bytes in front as zeros
    enc.seek(I * k + 5)
    tail = enc.process(message[I * k + 5:2 * I * k])
    zeroed = message[I * k:2 * I * k].copy()
    zeroed[:5] = 0
    assert np.array_equal(tail, rm.encode_frame(code, I, zeroed))


def test_pack_and_unpack():
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, 64).astype(np.uint8)
    assert rm.pack([1, 0, 0, 0, 0, 0, 1, 1]).tolist() == [0x83] and rm.pack([1, 0, 0, 0, 0, 0, 1, 1], msb=False).tolist() == [0xC1]
    assert rm.unpack([0x83]).tolist() == [1, 0, 0, 0, 0, 0, 1, 1] and rm.unpack([0x83], msb=False).tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    for msb in (True, False):
        assert np.array_equal(rm.pack(bits, msb), np.packbits(bits, bitorder="big" if msb else "little"))
        assert np.array_equal(rm.unpack(rm.pack(bits, msb), msb), bits)
        assert np.array_equal(rm.pack(bits | 0xFE, msb), rm.pack(bits, msb))                       # bit 0 is read
        model = rm.pack_model(msb)
        parts = [model.process(bits[a:b]) for a, b in zip([0, 3, 8, 9, 9], [3, 8, 9, 9, 64])]
        assert [len(p) for p in parts] == [0, 1, 0, 0, 7] and np.array_equal(np.concatenate(parts), rm.pack(bits, msb))
    model = rm.pack_model()
    assert model.seek(11) == 1 and model.memory() == 7
    assert model.process(bits[11:24]).tolist() == rm.pack(np.concatenate([[0, 0, 0], bits[11:16], bits[16:24]])).tolist()


# ---- rs_plan.h against Python integers and the model ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/host_rs_check.hip as plain C++; returns ask(lines) -> the answers, one list of integers per line"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rscheck")
    exe = str(d / "host_rs_check")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tools", "host_rs_check.hip")], capture_output=True, text=True, timeout=600)
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


FRAMES = [(223, 255), (255, 223), (5 * 255, 5 * 224), (8 * 253, 8 * 255), (8, 1), (1, 8), (188, 204), (8, 10)]


@pytest.mark.parametrize("fi,fo", FRAMES)
def test_counts_for_every_cut_of_a_short_stream_and_near_2_to_the_64(checker, fi, fo):
    top = (1 << 64) - 1
    qs = list(range(0, 3 * fi + 3, max(1, fi // 37))) + [fi - 1, fi, fi + 1, 2 * fi - 1, 2 * fi, top, top - 1, top - fi, (1 << 63) + 12345, (1 << 40) + 3]
    for q, (frames, held, ok, position) in zip(qs, checker(["done %d %d %d" % (fi, fo, q) for q in qs])):
        assert frames == q // fi and held == q % fi, q
        assert (ok, position) == ((1, frames * fo) if frames * fo < (1 << 64) else (0, 0)), q
    sizes = [0, 1, 2, fi - 1, fi, fi + 1, 3 * fi + 2, top, top - fi]
    for size, (bound,) in zip(sizes, checker(["max %d %d %d" % (fi, fo, s) for s in sizes])):
        assert bound == min(-(-size // fi) * fo, top), size
    assert checker(["shape %d %d" % (fi, fo)]) == [[fi - 1]]
    # max_output is never below the true count of a call, whatever was carried, and is reached
    rng = np.random.default_rng(fi)
    for _ in range(500):
        q, size = int(rng.integers(0, 4 * fi)), int(rng.integers(0, 3 * fi))
        assert ((q + size) // fi - q // fi) * fo <= -(-size // fi) * fo
    assert ((fi - 1 + 1) // fi - (fi - 1) // fi) * fo == fo == -(-1 // fi) * fo


def test_frames_of_the_stages(checker):
    cases = [(255, 223, 1, 0), (255, 223, 5, 1), (204, 188, 1, 1), (10, 8, 8, 0), (255, 191, 8, 1)]
    for (n, k, I, status), got in zip(cases, checker(["frames %d %d %d %d" % c for c in cases])):
        assert got == [I * k, I * n, I * n, I * (k + status)]


@pytest.mark.parametrize("name", list(SETS))
def test_tables_roots_generator_and_parity_against_the_model(checker, name):
    n, k, kw = SETS[name]
    code = rm.Code(n, k, **kw)
    args = "%d %d %d %d %d" % (n, k, code.gfpoly, code.fcr, code.prim)
    exp, roots, gen = checker(["exp " + args, "roots " + args, "gen " + args])
    assert exp == code.field.exp[:255] and exp[1] == 2 and exp[8] == code.gfpoly ^ 0x100
    assert roots == code.roots == root_values(n, k, **kw)
    assert gen == code.generator
    rows = sorted({0, 1, k // 2, k - 1})
    for i, row in zip(rows, checker(["parity %s %d" % (args, i) for i in rows])):
        assert row == code.parity(np.eye(1, k, i, dtype=np.int64)[0]), i


def test_every_primitive_polynomial_and_no_other(checker):
    polys = list(range(0x100, 0x200)) + [0xff, 0x200, 0x11d + 0x200, 0]
    got = checker(["check 255 223 %d 0 1 1" % p for p in polys])
    assert [p for p, (r,) in zip(polys, got) if r == 0] == list(rm.PRIMITIVE_POLYNOMIALS)
    assert all(r in (0, 3) for (r,) in got)
    assert [p for p in polys if lr.blocks.is_primitive_polynomial(p)] == list(rm.PRIMITIVE_POLYNOMIALS)
    cases = ["check 256 224 285 0 1 1", "check 2 0 285 0 1 1", "check 255 255 285 0 1 1", "check 255 222 285 0 1 1", "check 255 189 285 0 1 1",
             "check 255 0 285 0 1 1", "check 255 223 283 0 1 1", "check 255 223 285 255 1 1", "check 255 223 285 0 3 1", "check 255 223 285 0 0 1",
             "check 255 223 285 0 255 1", "check 255 223 285 0 1 0", "check 255 223 285 0 1 9", "check 255 191 391 112 11 8", "check 3 1 285 254 254 1"]
    assert [r for (r,) in checker(cases)] == [1, 1, 2, 2, 2, 2, 3, 4, 5, 5, 5, 6, 6, 0, 0]


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------------------
CODE_REFUSALS = [((256, 224, {}), "n must be 3 .. 255 (got 256)"), ((255, 255, {}), "n - k even and 2 .. 64 (got n = 255, k = 255)"),
                 ((255, 256, {}), "(got n = 255, k = 256)"), ((255, 222, {}), "n - k even and 2 .. 64 (got n = 255, k = 222)"),
                 ((255, 189, {}), "n - k even and 2 .. 64 (got n = 255, k = 189)"), ((255, 223, {"gfpoly": 0x11b}), "gfpoly 0x11b is not a primitive polynomial"),
                 ((255, 223, {"prim": 3}), "prim must be 1 .. 254 and coprime to 255 (got 3)"), ((255, 223, {"fcr": 255}), "fcr must be 0 .. 254 (got 255)"),
                 ((255, 223, {"fcr": -1}), "fcr must be 0 .. 254 (got -1)"), ((255, 223, {"interleave": 0}), "interleave must be 1 .. 8 (got 0)"),
                 ((255, 223, {"interleave": 9}), "interleave must be 1 .. 8 (got 9)")]


@pytest.mark.parametrize("cls,who", [(lr.ReedSolomonEncoderBlock, "rsenc"), (lr.ReedSolomonDecoderBlock, "rsdec")])
@pytest.mark.parametrize("args, fragment", CODE_REFUSALS, ids=[f for _, f in CODE_REFUSALS])
def test_defective_codes_are_refused(cls, who, args, fragment):
    with pytest.raises(ValueError) as e:
        cls(*args)
    assert str(e.value).startswith(who + ":") and fragment in str(e.value), str(e.value)
    # and by the library, in front of the device, with the same words, from a hand-written op string
    n, k, options = args
    fields = {"gfpoly": 0x11d, "fcr": 0, "prim": 1, "interleave": 1}
    fields.update(options)
    op = "%s:n=%d:k=%d:gfpoly=%d:fcr=%d:prim=%d:interleave=%d" % (who, n, k, fields["gfpoly"], fields["fcr"], fields["prim"], fields["interleave"])
    op += ":status=1" if who == "rsdec" else ""
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith(who + ":") and fragment in message, message


OP_REFUSALS = [("rsenc:n=255:k=223:gfpoly=285:fcr=0:prim=1:interleave=1:bogus=1", "unknown parameter \"bogus\""),
               ("rsenc:n=255:k=223:gfpoly=285:fcr=0:prim=1:interleave=1:status=1", "unknown parameter \"status\""),
               ("rsdec:n=255:k=223:gfpoly=285:fcr=0:prim=1:interleave=1", "missing parameter \"status\""),
               ("rsdec:n=255:k=223:gfpoly=285:fcr=0:prim=1:interleave=1:status=2", "status must be 0 or 1"),
               ("rsenc:n=255:k=223:gfpoly=0x11d:fcr=0:prim=1:interleave=1", "bad value for \"gfpoly\""),
               ("rsenc:n=255:k=223:fcr=0:prim=1:interleave=1", "missing parameter \"gfpoly\""),
               ("rsenc:n=255:gfpoly=285:fcr=0:prim=1:interleave=1", "missing parameter \"k\""),
               ("rsenc:n=99999999999:k=223:gfpoly=285:fcr=0:prim=1:interleave=1", "n must be 3 .. 255 (got 99999999999)"),
               ("packbits:order=middle", "unsupported order \"middle\" (msb or lsb)"), ("unpackbits:order=", "unsupported order \"\" (msb or lsb)"),
               ("packbits", "missing parameter \"order\""), ("unpackbits:order=msb:width=8", "unknown parameter \"width\"")]


@pytest.mark.parametrize("op, fragment", OP_REFUSALS, ids=[f for _, f in OP_REFUSALS])
def test_defective_op_strings_are_refused_in_front_of_the_device(op, fragment):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith(op.split(":")[0] + ":") and fragment in message, message


@pytest.mark.parametrize("make, fragment", [(lambda: lr.ReedSolomonEncoderBlock(255, 223, {"bogus": 1}), "rsenc: unknown option 'bogus'"),
                                            (lambda: lr.ReedSolomonEncoderBlock(255, 223, {"status": True}), "rsenc: unknown option 'status'"),
                                            (lambda: lr.ReedSolomonDecoderBlock(255.0, 223), "rsdec: n must be 3 .. 255 (got 255.0)"),
                                            (lambda: lr.ReedSolomonDecoderBlock(255, True), "(got n = 255, k = True)"),
                                            (lambda: lr.ReedSolomonDecoderBlock(255, 223, {"gfpoly": "0x11d"}), "gfpoly '0x11d' is not a primitive"),
                                            (lambda: lr.ReedSolomonDecoderBlock(255, 223, {"interleave": 2.0}), "interleave must be 1 .. 8 (got 2.0)"),
                                            (lambda: lr.PackBitsBlock({"order": "middle"}), "packbits: unsupported order 'middle' (msb or lsb)"),
                                            (lambda: lr.UnpackBitsBlock({"order": None, "x": 1}), "unpackbits: unknown option 'x'"),
                                            (lambda: lr.UnpackBitsBlock({"order": 1}), "unpackbits: unsupported order 1 (msb or lsb)")],
                         ids=["unknown option", "status on the encoder", "float n", "bool k", "text gfpoly", "float interleave", "bad order", "unknown pack option",
                              "order of the wrong kind"])
def test_arguments_of_the_wrong_kind_are_refused(make, fragment):
    with pytest.raises(ValueError) as e:
        make()
    assert fragment in str(e.value), str(e.value)


def test_op_strings_rates_and_types_of_the_blocks():
    """what the blocks hand to lrhip_unary_create: every field spelled out, gfpoly in decimal; the library has no complaint about the text (without a
    device its only refusal is the missing device)"""
    enc = lr.ReedSolomonEncoderBlock(204, 188)
    assert enc.op() == "rsenc:n=204:k=188:gfpoly=285:fcr=0:prim=1:interleave=1" and (enc.t, enc.frame_in, enc.frame_out, enc.memory()) == (8, 188, 204, 187)
    dec = lr.ReedSolomonDecoderBlock(255, 223, {"gfpoly": 0x187, "fcr": 112, "prim": 11, "interleave": 5, "status": True})
    assert dec.op() == "rsdec:n=255:k=223:gfpoly=391:fcr=112:prim=11:interleave=5:status=1"
    assert (dec.t, dec.frame_in, dec.frame_out, dec.memory()) == (16, 1275, 1120, 1274)
    plain = lr.ReedSolomonDecoderBlock(np.int64(10), np.int32(8))
    assert plain.op() == "rsdec:n=10:k=8:gfpoly=285:fcr=0:prim=1:interleave=1:status=0" and plain.frame_out == 8
    pack, unpack = lr.PackBitsBlock(), lr.UnpackBitsBlock({"order": "lsb"})
    assert pack.op() == "packbits:order=msb" and unpack.op() == "unpackbits:order=lsb" and (pack.memory(), unpack.memory()) == (7, 0)
    for blk, rate in ((enc, 188.0), (dec, 1275.0), (plain, 10.0), (pack, 8.0), (unpack, 1.0)):
        blk.rate = rate
    assert enc.get_rate() == 204.0 and dec.get_rate() == 1120.0 and plain.get_rate() == 8.0 and pack.get_rate() == 1.0 and unpack.get_rate() == 8.0
    for blk, in_type, out_type in ((enc, types.Byte, types.Byte), (dec, types.Byte, types.Byte), (pack, types.Bit, types.Byte), (unpack, types.Byte, types.Bit)):
        blk.differentiate([in_type])
        assert blk.get_output_type() is out_type
        L = _lib.load()
        ptr = L.lrhip_unary_create(blk.op().encode(), 0.0, 0.0, 0, 0)
        if ptr:
            L.lrhip_stage_destroy(ptr)
        else:
            assert not L.lrhip_strerror().decode().startswith(blk.op().split(":")[0] + ":"), L.lrhip_strerror().decode()
    with pytest.raises(TypeError):
        pack.differentiate([types.Float32])
