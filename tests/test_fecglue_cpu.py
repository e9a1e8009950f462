"""PunctureBlock, DepunctureBlock, ConvolutionalInterleaverBlock, ConvolutionalDeinterleaverBlock, AdditiveScramblerBlock and the DVB-S chain without
a device.  The models of tests/helpers/fecglue_model.py are the contract, so they are held to what the standards say of them - the first bytes of the
DVB and CCSDS sequences, the delay of an interleaver pair, the undelayed sync bytes - and to one another under every cut of a stream.  Then the header
luaradio_amd/csrc/fecglue_plan.h (tools/host_fecglue_check.hip, built for the host) against Python's integers, and the refusals of the blocks'
arguments and of the op strings, which need no device."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import _lib, types
from tests.helpers import fecglue_model as fm
from tests.helpers import op_string_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = list(fm.DVBS_PUNCTURE.values()) + ["10", "0" * 63 + "1", "1" + "0" * 63]
SHAPES = [(2, 1), (3, 5), (12, 17), (52, 4), (16, 256), (256, 1)]


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
def test_dvb_prbs_and_table():
    prbs = lr.lfsr_sequence((14, 15), fm.DVB_SEED, 64)
    assert prbs.dtype == np.uint8 and bytes(prbs).hex() == "03f6083430b8a393"
    table = lr.dvb_energy_dispersal_table()
    assert table.dtype == np.uint8 and len(table) == 1504 and zlib.crc32(bytes(table)) == 0x3427e129
    assert bytes(table[186:190]).hex() == "c5ba009f" and table[0] == 0xFF and bytes(table[1:9]).hex() == "03f6083430b8a393"
    assert all(table[188 * q] == 0 for q in range(1, 8))
    assert np.array_equal(table, fm.dvb_energy_dispersal_table()) and np.array_equal(table, lr.dvb_energy_dispersal_table(188))
    # frame 189: the same 188 entries per frame, a zero behind them; the PRBS does not advance over it
    wide = lr.dvb_energy_dispersal_table(189)
    assert len(wide) == 1512 and np.array_equal(wide.reshape(8, 189)[:, :188], table.reshape(8, 188)) and not wide.reshape(8, 189)[:, 188].any()
    assert np.array_equal(wide, fm.dvb_energy_dispersal_table(189))
    # the sync byte of the first packet of a period is inverted, the seven others are left alone
    packets = fm.ts_packets(np.random.default_rng(1), 9)
    sent = fm.ScramblerModel(table).process(packets)
    assert sent[::188].tolist() == [0xB8] + [0x47] * 7 + [0xB8]
    with pytest.raises(ValueError):
        lr.dvb_energy_dispersal_table(204)


def test_ccsds_table_and_lfsr_sequence():
    table = lr.ccsds_randomizer_table(255)
    assert bytes(table[:5]).hex() == "ff480ec09a" and np.array_equal(table, fm.ccsds_randomizer_table(255))
    bits = np.unpackbits(lr.ccsds_randomizer_table(64))
    assert np.array_equal(bits[255:510], bits[:255]) and not np.array_equal(bits[1:256], bits[:255])           # the period is 255 bits
    assert np.array_equal(lr.ccsds_randomizer_table(10), table[:10])
    # the definition, literally: s[m] = xor of s[m - i], seed_bits[i - 1] = s[-i], MSB first
    assert lr.lfsr_sequence((1,), [1], 8).tolist() == [0xFF] and lr.lfsr_sequence((2,), [1, 0], 8).tolist() == [0x55]
    assert lr.lfsr_sequence((1, 2), [1, 0], 16).tolist() == fm.lfsr_sequence((1, 2), [1, 0], 16).tolist() == [0xB6, 0xDB]
    for bad in (lambda: lr.lfsr_sequence((14, 15), [1] * 14, 8), lambda: lr.lfsr_sequence((1,), [1], 12), lambda: lr.ccsds_randomizer_table(0),
                lambda: lr.ccsds_randomizer_table(8193)):
        with pytest.raises(ValueError):
            bad()


# ---- the models against what is known of them -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,M", SHAPES)
def test_interleaver_pair_is_a_delay_of_D(I, M):
    D = (I - 1) * M * I
    rng = np.random.default_rng(I * M)
    n = min(2 * D + 3 * I + 7, 6000 + D)
    x = rng.integers(1, 256, n).astype(np.uint8)                   # no zero byte: a zero out is a FIFO's fill
    mid = fm.ConvolutionalInterleaverModel(I, M).process(x)
    back = fm.ConvolutionalInterleaverModel(I, M, True).process(mid)
    assert not back[:D].any() and np.array_equal(back[D:], x[:n - D])
    assert np.array_equal(mid[::I], x[::I])                        # branch 0 is not delayed
    assert np.array_equal(mid, fm.interleave_fast(x, I, M)) and np.array_equal(back, fm.interleave_fast(mid, I, M, True))
    assert fm.ConvolutionalInterleaverModel(I, M).memory() == D


def test_dvb_interleaver_delay_and_sync_bytes():
    model, inverse = fm.ConvolutionalInterleaverModel(12, 17), fm.ConvolutionalInterleaverModel(12, 17, True)
    assert model.D == 2244 == 11 * 204
    x = np.random.default_rng(2).integers(0, 256, 30 * 204).astype(np.uint8)
    x[::204] = 0x47
    mid = model.process(x)
    assert (mid[::204] == 0x47).all()                              # 204 = 12 * 17: the sync bytes ride branch 0
    back = inverse.process(mid)
    assert np.array_equal(back[2244:], x[:-2244]) and not back[:2244].any()
    # byte 1 of a packet is delayed by 17 * 12 bytes, one packet
    assert mid[204 + 1] == x[1] and mid[1] == 0


@pytest.mark.parametrize("rate", list(fm.DVBS_PUNCTURE))
def test_depuncture_of_puncture(rate):
    pattern = fm.DVBS_PUNCTURE[rate]
    num, den = [int(v) for v in rate.split("/")]
    assert pattern.count("1") * num == len(pattern) // 2 * den                          # len / 2 message bits, popcount code bits
    x = np.arange(1, 5 * len(pattern) + 1).astype(np.float32)
    y = fm.depuncture_model(pattern).process(fm.puncture_model(pattern).process(x.astype(np.uint8)).astype(np.float32))
    keep = np.array([c == "1" for c in pattern] * 5)
    assert np.array_equal(y[keep], x[keep]) and not y[~keep].any() and not np.signbit(y[~keep]).any()
    bits = np.random.default_rng(3).integers(0, 256, 3 * pattern.count("1")).astype(np.uint8)
    hard = fm.depuncture_model(pattern, False).process(bits)
    assert np.array_equal(hard[keep[:len(hard)]], 1.0 - 2.0 * (bits & 1)) and not hard[~keep[:len(hard)]].any()


def test_depuncture_moves_the_bits_of_an_llr():
    odd = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x00000001, 0x7F800000], np.uint32).view(np.float32)
    out = fm.depuncture_model("110110").process(np.concatenate([odd, odd[:3]]))
    assert out.view(np.uint32).tolist() == [0x7FC00001, 0xFFC12345, 0, 0x80000000, 0x00000001, 0, 0x7F800000, 0x7FC00001, 0, 0xFFC12345, 0x80000000, 0]


def cuts_of(n):
    return [[n], [1] * n, [0, 3, 0, n - 3], [n - 1, 1], [5, 0, 0, 7, n - 12]]


def test_models_under_every_cut_agree_with_one_call():
    rng = np.random.default_rng(4)
    table = rng.integers(0, 256, 7).astype(np.uint8)
    cases = [(lambda: fm.puncture_model("1101100110"), rng.integers(0, 2, 73).astype(np.uint8)),
             (lambda: fm.depuncture_model("11010101100110"), rng.standard_normal(61).astype(np.float32)),
             (lambda: fm.depuncture_model("10", False), rng.integers(0, 2, 40).astype(np.uint8)),
             (lambda: fm.ConvolutionalInterleaverModel(3, 5), rng.integers(0, 256, 90).astype(np.uint8)),
             (lambda: fm.ConvolutionalInterleaverModel(4, 2, True), rng.integers(0, 256, 70).astype(np.uint8)),
             (lambda: fm.ScramblerModel(table, 3), rng.integers(0, 256, 50).astype(np.uint8))]
    for make, x in cases:
        whole = make().process(x)
        for sizes in cuts_of(len(x)) + [[a, len(x) - a] for a in range(1, len(x))]:
            m = make()
            parts = [m.process(x[a:a + s]) for a, s in zip(np.cumsum([0] + sizes[:-1]), sizes)]
            got = np.concatenate(parts)
            assert got.dtype == whole.dtype and np.array_equal(got.view(np.uint8), whole.view(np.uint8)), sizes
        # a seek continues at the absolute index with zeros in front
        m = make()
        n0 = 17
        m.seek(n0)
        tail = m.process(x[n0:])
        if isinstance(m, fm.FramedModel):
            zeroed = x.copy()
            zeroed[n0 - n0 % m.fi:n0] = 0
            assert np.array_equal(tail.view(np.uint8), make().process(zeroed)[(n0 // m.fi) * m.fo:].view(np.uint8))
        elif isinstance(m, fm.ScramblerModel):
            assert np.array_equal(tail, whole[n0:])
        else:
            zeroed = x.copy()
            zeroed[:n0] = 0
            assert np.array_equal(tail, make().process(zeroed)[n0:])
    far = fm.ScramblerModel(table, 3)
    far.seek((1 << 70) + 5)
    assert np.array_equal(fm.scramble_fast(x, table, 3, (1 << 70) + 5), far.process(x))


def test_dvbs_chain_model_clean_loopback():
    """the chain of models: 11 packets of fill, then the packets; the descrambler's offset of five frames meets packet 0 with entry 0"""
    rate, count = "7/8", 9
    packets = fm.ts_packets(np.random.default_rng(5), count + fm.DVBS_FILL_PACKETS + 1)
    bits = fm.dvbs_encoder_model(rate).process(packets)
    assert len(bits) == len(packets) // 188 * 204 * 8 * 2 * 8 // 14
    llr = np.concatenate([1.0 - 2.0 * bits.astype(np.float32), np.zeros(2 * (64 + 32), np.float32)])
    out = fm.dvbs_decoder_model(rate, block=64, depth=32).process(llr)
    assert len(out) >= (count + fm.DVBS_FILL_PACKETS) * 188
    assert np.array_equal(out[fm.DVBS_FILL_PACKETS * 188:(fm.DVBS_FILL_PACKETS + count) * 188], packets[:count * 188])
    hard = fm.dvbs_decoder_model(rate, soft=False, status=True, block=64, depth=32).process(np.concatenate([bits, np.zeros(8 * 14, np.uint8)]))
    frames = hard[:len(hard) // 189 * 189].reshape(-1, 189)[fm.DVBS_FILL_PACKETS:]
    assert len(frames) >= 6 and np.array_equal(frames[:6, :188].ravel(), packets[:6 * 188]) and not frames[:6, 188].any()


# ---- fecglue_plan.h against Python integers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/host_fecglue_check.hip as plain C++; returns ask(lines) -> the answers, one list of integers per line"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("fgcheck")
    exe = str(d / "host_fecglue_check")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tools", "host_fecglue_check.hip")], capture_output=True, text=True, timeout=600)
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


TOP = (1 << 64) - 1


def test_patterns_frames_and_maps(checker):
    for pattern, (check, pfi, pfo, dfi, dfo) in zip(PATTERNS, checker(["frames " + p for p in PATTERNS])):
        assert (check, pfi, pfo, dfi, dfo) == (0, len(pattern), pattern.count("1"), pattern.count("1"), len(pattern))
    for pattern, pmap, dmap in zip(PATTERNS, checker(["pmap " + p for p in PATTERNS]), checker(["dmap " + p for p in PATTERNS])):
        assert pmap == [j for j, c in enumerate(pattern) if c == "1"]
        assert dmap == [pattern[:j].count("1") if c == "1" else 255 for j, c in enumerate(pattern)]
        frame = np.arange(100, 100 + len(pattern)).astype(np.uint8)
        assert fm.puncture_frame(pattern, frame).tolist() == [int(frame[j]) for j in pmap]
    bad = ["1", "", "1" * 65, "0" * 64, "00", "1201", "1a", "1" * 64, "01"]
    assert [r[0] for r in checker(["frames " + p for p in bad])] == [1, 1, 1, 3, 3, 2, 2, 0, 0]


@pytest.mark.parametrize("pattern", ["110110", "11010101100110", "0" * 63 + "1", "11"])
def test_counts_in_elements_for_every_cut_and_near_2_to_the_64(checker, pattern):
    for fi, fo in ((len(pattern), pattern.count("1")), (pattern.count("1"), len(pattern))):
        qs = list(range(0, 3 * fi + 3)) + [TOP, TOP - 1, TOP - fi, (1 << 63) + 12345, (1 << 40) + 3]
        for q, (frames, held, ok, position) in zip(qs, checker(["done %d %d %d" % (fi, fo, q) for q in qs])):
            assert frames == q // fi and held == q % fi, q
            assert (ok, position) == ((1, frames * fo) if frames * fo < (1 << 64) else (0, 0)), q
        sizes = [0, 1, 2, fi - 1, fi, fi + 1, 3 * fi + 2, TOP, TOP - fi]
        for size, (bound,) in zip(sizes, checker(["max %d %d %d" % (fi, fo, s) for s in sizes])):
            assert bound == min(-(-size // fi) * fo, TOP), size
        assert checker(["shape %d %d" % (fi, fo)]) == [[fi - 1]]
        # the model counts the same way
        model = fm.FramedModel(fi, fo, lambda frame: np.zeros(fo, np.uint8))
        assert model.seek((1 << 40) + 3) == (((1 << 40) + 3) // fi) * fo and len(model.held) == ((1 << 40) + 3) % fi and model.memory() == fi - 1


def test_table_index_never_wraps(checker):
    cases = [(i, K, P) for P in (1, 7, 255, 1504, 1512, 8192) for K in sorted({0, P // 2, P - 1})
             for i in (0, 1, P - 1, P, P + 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3, (1 << 63) + 5, TOP - 1, TOP)]
    for (i, K, P), (index,) in zip(cases, checker(["table %d %d %d" % c for c in cases])):
        assert index == (i + K) % P, (i, K, P)
    steps = [(t, n, P) for P in (1, 7, 1504, 8192) for t in sorted({0, P - 1}) for n in (0, 1, P, P + 1, (1 << 32) + 1, TOP)]
    for (t, n, P), (index,) in zip(steps, checker(["advance %d %d %d" % s for s in steps])):
        assert index == (t + n) % P, (t, n, P)


def test_interleaver_shapes_and_source_index(checker):
    shapes = SHAPES + [(1, 1), (257, 1), (2, 0), (2, 257), (256, 2), (17, 241), (17, 240), (256, 1), (2, 256), (0, 0)]
    for (I, M), (check, depth) in zip(shapes, checker(["check %d %d" % s for s in shapes])):
        want = 1 if not 2 <= I <= 256 else 2 if not 1 <= M <= 256 else 3 if (I - 1) * M * I > 65536 else 0
        assert (check, depth) == (want, 0 if want else (I - 1) * M * I), (I, M)
        if not want:
            fm.check_interleaver(I, M)
        else:
            with pytest.raises(ValueError):
                fm.check_interleaver(I, M)
    for I, M in SHAPES:
        D = (I - 1) * M * I
        spots = sorted({0, 1, I - 1, I, M * I, M * I + 1, D - 1, D, D + 1, D + I - 1, 2 * D + 5, (1 << 40) + 3, (1 << 63) + 7, TOP - I, TOP - 1, TOP})
        for deint in (0, 1):
            for i, (ok, src) in zip(spots, checker(["source %d %d %d %d" % (i, I, M, deint) for i in spots])):
                want = i - fm.interleaver_delay(i, I, M, bool(deint))
                assert (ok, src) == ((1, want) if want >= 0 else (0, 0)), (i, I, M, deint)


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------------------
HEX = "00ff10"
OP_REFUSALS = [("puncture", "missing parameter \"pattern\""), ("puncture:pattern=", "pattern must be 2 .. 64 characters (got 0)"),
               ("puncture:pattern=1", "pattern must be 2 .. 64 characters (got 1)"), ("puncture:pattern=" + "1" * 65, "pattern must be 2 .. 64 characters (got 65)"),
               ("puncture:pattern=0000", "pattern must not be all 0"), ("puncture:pattern=1201", "pattern must be a string of 0 / 1 characters"),
               ("puncture:pattern=11:input=llr", "unknown parameter \"input\""), ("puncture:pattern=11:pattern=11", "parameter \"pattern\" given twice"),
               ("puncture:pattern", "malformed parameter"),
               ("depuncture:pattern=110110", "missing parameter \"input\""), ("depuncture:input=llr", "missing parameter \"pattern\""),
               ("depuncture:pattern=110110:input=soft", "unsupported input \"soft\" (llr or bit)"), ("depuncture:pattern=110110:input=", "unsupported input \"\""),
               ("depuncture:pattern=00:input=bit", "pattern must not be all 0"), ("depuncture:pattern=1x:input=bit", "pattern must be a string of 0 / 1"),
               ("depuncture:pattern=11:input=bit:bogus=1", "unknown parameter \"bogus\""),
               ("convinterleave:branches=12", "missing parameter \"step\""), ("convinterleave:step=17", "missing parameter \"branches\""),
               ("convinterleave:branches=1:step=17", "branches must be 2 .. 256 (got 1)"), ("convinterleave:branches=257:step=1", "branches must be 2 .. 256 (got 257)"),
               ("convinterleave:branches=12:step=0", "step must be 1 .. 256 (got 0)"), ("convinterleave:branches=12:step=257", "step must be 1 .. 256 (got 257)"),
               ("convinterleave:branches=256:step=2", "the depth (branches - 1) * step * branches = 130560 must be at most 65536"),
               ("convinterleave:branches=12.5:step=17", "bad value for \"branches\""), ("convinterleave:branches=12:step=x", "bad value for \"step\""),
               ("convinterleave:branches=12:step=17:depth=2244", "unknown parameter \"depth\""),
               ("convdeinterleave:branches=12", "missing parameter \"step\""), ("convdeinterleave:branches=0:step=1", "branches must be 2 .. 256 (got 0)"),
               ("convdeinterleave:branches=17:step=241", "must be at most 65536"), ("convdeinterleave:branches=12:step=-1", "step must be 1 .. 256 (got -1)"),
               ("convdeinterleave:branches=12:step=17:", "malformed parameter"),
               ("scrambler:offset=0", "missing parameter \"table\""), ("scrambler:table=" + HEX, "missing parameter \"offset\""),
               ("scrambler:table=:offset=0", "table must be an even number of hexadecimal digits"),
               ("scrambler:table=0ff:offset=0", "table must be an even number of hexadecimal digits"),
               ("scrambler:table=0g:offset=0", "table must be an even number of hexadecimal digits"),
               ("scrambler:table=0x00:offset=0", "table must be an even number of hexadecimal digits"),
               ("scrambler:table=" + "00" * 8193 + ":offset=0", "the table has 8193 bytes, it must be 1 .. 8192"),
               ("scrambler:table=" + HEX + ":offset=3", "offset must be 0 .. 2"), ("scrambler:table=" + HEX + ":offset=-1", "offset must be 0 .. 2"),
               ("scrambler:table=" + HEX + ":offset=1.5", "bad value for \"offset\""), ("scrambler:table=" + HEX + ":offset=0:seed=1", "unknown parameter \"seed\"")]
OP_WELL_FORMED = (["puncture:pattern=" + p for p in PATTERNS] + ["depuncture:pattern=%s:input=%s" % (p, i) for p in PATTERNS[:3] for i in ("llr", "bit")] +
                  ["depuncture:input=bit:pattern=10"] + ["%s:branches=%d:step=%d" % (h, I, M) for h in ("convinterleave", "convdeinterleave") for I, M in SHAPES] +
                  ["convinterleave:branches=17:step=240", "scrambler:table=00:offset=0", "scrambler:table=aBcDeF:offset=2", "scrambler:offset=8191:table=" + "5a" * 8192])


@pytest.mark.parametrize("op, fragment", OP_REFUSALS, ids=["%s-%d" % (op.split(":")[0], i) for i, (op, _) in enumerate(OP_REFUSALS)])
def test_defective_op_strings_are_refused_in_front_of_the_device(op, fragment):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    message = L.lrhip_strerror().decode()
    assert message.startswith(op.split(":")[0] + ":") and fragment in message, message
    assert not C.accepted(message)                                 # a message of the readers, by the conventions of the op-string corpus


@pytest.mark.parametrize("op", OP_WELL_FORMED, ids=[op[:40] for op in OP_WELL_FORMED])
def test_well_formed_op_strings_get_past_the_readers(op):
    rejected, message = C.ask(_lib.load(), op)
    assert not rejected or C.accepted(message), message


BLOCK_REFUSALS = [(lambda: lr.PunctureBlock("1"), "puncture: pattern must be 2 .. 64 characters (got 1)"),
                  (lambda: lr.PunctureBlock("1" * 65), "puncture: pattern must be 2 .. 64 characters (got 65)"),
                  (lambda: lr.PunctureBlock("0000"), "puncture: pattern must not be all 0"),
                  (lambda: lr.PunctureBlock("1201"), "puncture: pattern must be a string of 0 / 1 characters"),
                  (lambda: lr.PunctureBlock(0b1101), "puncture: pattern must be a string of 0 / 1 characters"),
                  (lambda: lr.DepunctureBlock("00"), "depuncture: pattern must not be all 0"),
                  (lambda: lr.DepunctureBlock("11", {"hard": True}), "depuncture: unknown option 'hard'"),
                  (lambda: lr.ConvolutionalInterleaverBlock(1, 17), "convinterleave: branches must be 2 .. 256 (got 1)"),
                  (lambda: lr.ConvolutionalInterleaverBlock(12.0, 17), "convinterleave: branches must be 2 .. 256 (got 12.0)"),
                  (lambda: lr.ConvolutionalInterleaverBlock(12, 257), "convinterleave: step must be 1 .. 256 (got 257)"),
                  (lambda: lr.ConvolutionalDeinterleaverBlock(12, 0), "convdeinterleave: step must be 1 .. 256 (got 0)"),
                  (lambda: lr.ConvolutionalDeinterleaverBlock(256, 2), "convdeinterleave: the depth (branches - 1) * step * branches = 130560 must be at most 65536"),
                  (lambda: lr.ConvolutionalDeinterleaverBlock(True, 2), "convdeinterleave: branches must be 2 .. 256 (got True)"),
                  (lambda: lr.AdditiveScramblerBlock([]), "scrambler: the table must be a vector of integers 0 .. 255"),
                  (lambda: lr.AdditiveScramblerBlock([1, 256]), "scrambler: the table must be a vector of integers 0 .. 255"),
                  (lambda: lr.AdditiveScramblerBlock([0.5]), "scrambler: the table must be a vector of integers 0 .. 255"),
                  (lambda: lr.AdditiveScramblerBlock(np.zeros(8193, np.uint8)), "scrambler: the table has 8193 bytes, it must be 1 .. 8192"),
                  (lambda: lr.AdditiveScramblerBlock([1, 2, 3], {"offset": 3}), "scrambler: offset must be 0 .. 2"),
                  (lambda: lr.AdditiveScramblerBlock([1, 2, 3], {"offset": -1}), "scrambler: offset must be 0 .. 2"),
                  (lambda: lr.AdditiveScramblerBlock([1, 2, 3], {"seed": 1}), "scrambler: unknown option 'seed'")]


@pytest.mark.parametrize("make, fragment", BLOCK_REFUSALS, ids=[f[:60] for _, f in BLOCK_REFUSALS])
def test_the_blocks_refuse_the_same_domains(make, fragment):
    with pytest.raises(ValueError) as e:
        make()
    assert fragment in str(e.value), str(e.value)


def test_op_strings_rates_types_and_memory_of_the_blocks():
    punct, soft, hard = lr.PunctureBlock("110110"), lr.DepunctureBlock("110110"), lr.DepunctureBlock("1101", {"soft": False})
    inter, deinter = lr.ConvolutionalInterleaverBlock(12, 17), lr.ConvolutionalDeinterleaverBlock(np.int64(52), np.int32(4))
    scr = lr.AdditiveScramblerBlock(np.array([0, 255, 16], np.uint8), {"offset": 2})
    assert punct.op() == "puncture:pattern=110110" and (punct.frame_in, punct.frame_out, punct.memory()) == (6, 4, 5)
    assert soft.op() == "depuncture:pattern=110110:input=llr" and (soft.frame_in, soft.frame_out, soft.memory()) == (4, 6, 3)
    assert hard.op() == "depuncture:pattern=1101:input=bit" and (hard.frame_in, hard.frame_out, hard.memory()) == (3, 4, 2)
    assert inter.op() == "convinterleave:branches=12:step=17" and inter.memory() == inter.depth == 2244
    assert deinter.op() == "convdeinterleave:branches=52:step=4" and deinter.memory() == 51 * 4 * 52
    assert scr.op() == "scrambler:table=00ff10:offset=2" and scr.memory() == 0
    assert lr.AdditiveScramblerBlock(lr.dvb_energy_dispersal_table()).op().startswith("scrambler:table=ff03f608") and len(lr.AdditiveScramblerBlock(
        lr.dvb_energy_dispersal_table(189), {"offset": 945}).op()) == len("scrambler:table=:offset=945") + 2 * 1512
    for blk in (punct, soft, hard, inter, deinter, scr):
        blk.rate = 12.0
    assert [b.get_rate() for b in (punct, soft, hard, inter, deinter, scr)] == [8.0, 18.0, 16.0, 12.0, 12.0, 12.0]
    L = _lib.load()
    for blk, in_type, out_type in ((punct, types.Bit, types.Bit), (soft, types.Float32, types.Float32), (hard, types.Bit, types.Float32),
                                   (inter, types.Byte, types.Byte), (deinter, types.Byte, types.Byte), (scr, types.Byte, types.Byte)):
        blk.differentiate([in_type])
        assert blk.get_output_type() is out_type
        rejected, message = C.ask(L, blk.op())
        assert not rejected or C.accepted(message), message
    with pytest.raises(TypeError):
        soft.differentiate([types.Bit])
    with pytest.raises(TypeError):
        hard.differentiate([types.Float32])


def test_dvbs_composites_without_a_device():
    assert lr.DVBS_PUNCTURE == fm.DVBS_PUNCTURE and lr.DVBS_FILL_PACKETS == fm.DVBS_FILL_PACKETS == 11 and set(lr.DVBS_DEPTH) == set(lr.DVBS_PUNCTURE)
    assert all(d % 16 == 0 and 16 <= d <= 256 for d in lr.DVBS_DEPTH.values())
    for make in (lambda: lr.dvbs_fec_decoder("4/5"), lambda: lr.dvbs_fec_encoder("1/3"), lambda: lr.dvbs_fec_decoder(rate=0.75)):
        with pytest.raises(ValueError) as e:
            make()
        assert "Unsupported DVB-S code rate" in str(e.value)
    tx = lr.dvbs_fec_encoder_blocks("2/3")
    assert [b.op() for b in tx[1:]] == ["rsenc:n=204:k=188:gfpoly=285:fcr=0:prim=1:interleave=1", "convinterleave:branches=12:step=17", "unpackbits:order=msb",
                                        "convenc:k=7:polys=171,133", "puncture:pattern=1101"]
    assert tx[0].offset == 0 and np.array_equal(tx[0].table, fm.dvb_energy_dispersal_table(188))
    rx = lr.dvbs_fec_decoder_blocks("5/6", status=True)
    assert [b.op() for b in rx[:5]] == ["depuncture:pattern=1101100110:input=llr", "viterbi:k=7:polys=171,133:input=llr:scale=8:block=512:depth=%d" % lr.DVBS_DEPTH["5/6"],
                                        "packbits:order=msb", "convdeinterleave:branches=12:step=17", "rsdec:n=204:k=188:gfpoly=285:fcr=0:prim=1:interleave=1:status=1"]
    assert rx[5].offset == 5 * 189 and np.array_equal(rx[5].table, fm.dvb_energy_dispersal_table(189))
    hard = lr.dvbs_fec_decoder_blocks("1/2", soft=False, block=256, depth=64)
    assert hard[0].op() == "depuncture:pattern=11:input=bit" and hard[1].op() == "viterbi:k=7:polys=171,133:input=llr:scale=127:block=256:depth=64"
    assert hard[5].offset == 5 * 188 and len(hard[5].table) == 1504
