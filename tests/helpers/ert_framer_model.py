"""Models of the reference's three ERT framers - radio/blocks/protocol/scmframer.lua, scmplusframer.lua, idmframer.lua - for the tests of
SCMFramerBlock, SCMPlusFramerBlock and IDMFramerBlock.

FramerLiteral is each process() loop as written: a shift buffer of L bytes, tested whenever it is full, emptied by an accepted frame, and
*corrected in place*: scm_plus_correct_codeword and idm_correct_codeword flip the erroneous byte inside the buffer before the remaining
checks run, so a window that corrects and then fails a later check leaves its flip behind for every later window that still holds the byte.
pure_window_walk is the walk that ignores this (every window judged on the raw bytes).  The encoders build valid frames from field values, and
persistent_case builds the stream on which the two differ.

Byte semantics, as in the reference: Bit.tonumber / tobytes and the syndrome loops count a byte as 1 only when it equals 1; Bit:bnot turns a
byte b into (~b) & 1; idm_compute_crc (idmframer.lua:140-154) compares (crc & 0x8000) ^ (b << 15) with 0x8000, so there a byte of 1 is a one, a
byte of 0 is a zero and a byte of 2 or more never takes the XOR branch."""
import numpy as np

from luaradio_amd import types


def _poly_rows(n, poly):
    """row i = x^(n - 1 - i) mod the 16-bit generator `poly` (its x^16 term implied): the reference's SCM_CHECK_SYNDROMES (scmframer.lua:53-73)
    and SCM_PLUS_CHECK_SYNDROMES (scmplusframer.lua:51-80), which end in the identity"""
    rows, r = [0] * n, 1
    for i in range(n - 1, -1, -1):
        rows[i] = r
        r <<= 1
        if r & 0x10000:
            r ^= 0x10000 | poly
    return rows


def idm_crc(buf, offset, length):
    """idm_compute_crc, on raw bytes"""
    crc = 0xffff
    for i in range(length):
        if ((crc & 0x8000) ^ (int(buf[offset + i]) << 15)) == 0x8000:
            crc = ((crc << 1) ^ 0x1021) & 0xffffffff
        else:
            crc = (crc << 1) & 0xffffffff
    return (crc ^ 0xffff) & 0xffff


def _idm_rows():
    """idm_initialize_crc (idmframer.lua:156-176)"""
    vec = bytearray(704 - 16)
    rows = []
    for i in range(len(vec)):
        vec[i] = 1
        rows.append(idm_crc(vec, 0, len(vec)) ^ 0x866b)
        vec[i] = 0
    return rows + [1 << (15 - i) for i in range(16)]


def tonumber(buf, offset, length):
    v = 0
    for b in buf[offset:offset + length]:
        v = (v << 1) | (1 if b == 1 else 0)
    return v


def tobytes(buf, offset, length):
    return [tonumber(buf, offset + i, 8) for i in range(0, length, 8)]


_ONES = bytes(1 if b == 1 else 0 for b in range(256))


class Protocol:
    def __init__(self, name, frame_len, pre_bits, pre_value, cw_len, init, rows, sample_type):
        self.name, self.L, self.pre_bits, self.pre_value, self.cw_off, self.cw_len, self.init = name, frame_len, pre_bits, pre_value, pre_bits, cw_len, init
        self.rows = rows
        self.correct = {}
        for i, r in enumerate(rows):                     # the reference's CORRECT_SYNDROMES: on equal rows the later index would win
            self.correct[r] = i
        self.sample_type, self.dtype = sample_type, sample_type.dtype
        self.pre_bytes = bytes((pre_value >> (pre_bits - 1 - i)) & 1 for i in range(pre_bits))
        assert frame_len == pre_bits + cw_len and len(rows) == cw_len

    def preamble(self):
        return np.frombuffer(self.pre_bytes, np.uint8).copy()

    def syndrome(self, buf):
        s = self.init
        for i in range(self.cw_len):
            if buf[self.cw_off + i] == 1:
                s ^= self.rows[i]
        return s

    def correct_codeword(self, buf):
        """*_correct_codeword: True / False, the flip made in `buf`"""
        s = self.syndrome(buf)
        if s == 0:
            return True
        k = self.correct.get(s)
        if k is not None:
            buf[self.cw_off + k] = (~buf[self.cw_off + k]) & 1
            return True
        return False

    def try_frame(self, buf):
        """the body of `if frame_length == FRAME_LEN` on a full buffer (a bytearray, corrected in place): the record's fields or None"""
        if bytes(buf[:self.pre_bits]).translate(_ONES) != self.pre_bytes:
            return None
        if not self.correct_codeword(buf):
            return None
        return self.fields(buf)

    def records(self, frames):
        """the structured array of a list of field dicts; the pad bytes are zero"""
        rec = np.zeros(len(frames), self.dtype)
        for i, f in enumerate(frames):
            for k, v in f.items():
                rec[k][i] = v
        return rec

    def record(self, fields):
        return self.records([fields])


class _SCM(Protocol):
    def fields(self, buf):
        return dict(ert_type=tonumber(buf, 26, 4), ert_id=(tonumber(buf, 21, 2) << 24) | tonumber(buf, 56, 24), consumption=tonumber(buf, 32, 24),
                    physical_tamper=tonumber(buf, 24, 2), encoder_tamper=tonumber(buf, 30, 2), reserved=tonumber(buf, 23, 1), crc=tonumber(buf, 80, 16))

    golden_order = ("ert_type", "ert_id", "consumption", "physical_tamper", "encoder_tamper", "reserved", "crc")

    def message(self, ert_type=0, ert_id=0, consumption=0, physical_tamper=0, encoder_tamper=0, reserved=0):
        return _bits(ert_id >> 24, 2) + _bits(reserved, 1) + _bits(physical_tamper, 2) + _bits(ert_type, 4) + _bits(encoder_tamper, 2) + \
            _bits(consumption, 24) + _bits(ert_id & 0xffffff, 24)

    def random_fields(self, rng):
        return dict(ert_type=int(rng.integers(16)), ert_id=int(rng.integers(1 << 26)), consumption=int(rng.integers(1 << 24)),
                    physical_tamper=int(rng.integers(4)), encoder_tamper=int(rng.integers(4)), reserved=int(rng.integers(2)))


class _SCMPlus(Protocol):
    def fields(self, buf):
        protocol_id = tonumber(buf, 16, 8)
        if protocol_id != 0x1e:
            return None
        return dict(protocol_id=protocol_id, ert_type=tonumber(buf, 24, 8), ert_id=tonumber(buf, 32, 32), consumption=tonumber(buf, 64, 32),
                    tamper=tonumber(buf, 96, 16), crc=tonumber(buf, 112, 16))

    golden_order = ("protocol_id", "ert_type", "ert_id", "consumption", "tamper", "crc")

    def message(self, protocol_id=0x1e, ert_type=0, ert_id=0, consumption=0, tamper=0):
        return _bits(protocol_id, 8) + _bits(ert_type, 8) + _bits(ert_id, 32) + _bits(consumption, 32) + _bits(tamper, 16)

    def random_fields(self, rng):
        return dict(protocol_id=0x1e, ert_type=int(rng.integers(256)), ert_id=int(rng.integers(1 << 32)), consumption=int(rng.integers(1 << 32)),
                    tamper=int(rng.integers(1 << 16)))


class _IDM(Protocol):
    def fields(self, buf):
        packet_type, packet_length, serial_crc = tonumber(buf, 32, 8), tonumber(buf, 40, 16), tonumber(buf, 704, 16)
        if not (packet_type == 0x1c and packet_length == 0x5cc6 and serial_crc == idm_crc(buf, 72, 32)):
            return None
        return dict(application_version=tonumber(buf, 56, 8), ert_type=tonumber(buf, 64, 8), ert_id=tonumber(buf, 72, 32),
                    consumption_interval_count=tonumber(buf, 104, 8), module_programming_state=tonumber(buf, 112, 8),
                    tamper_count=tobytes(buf, 120, 48), async_count=tobytes(buf, 168, 16), power_outage_flags=tobytes(buf, 184, 48),
                    last_consumption_count=tonumber(buf, 232, 32), differential_consumption_intervals=tobytes(buf, 264, 424),
                    transmit_time_offset=tonumber(buf, 688, 16), serial_crc=serial_crc, packet_crc=tonumber(buf, 720, 16))

    golden_order = ("application_version", "ert_type", "ert_id", "consumption_interval_count", "module_programming_state", "tamper_count",
                    "async_count", "power_outage_flags", "last_consumption_count", "differential_consumption_intervals", "transmit_time_offset",
                    "serial_crc", "packet_crc")

    def message(self, packet_type=0x1c, packet_length=0x5cc6, application_version=0, ert_type=0, ert_id=0, consumption_interval_count=0,
                module_programming_state=0, tamper_count=(0,) * 6, async_count=(0,) * 2, power_outage_flags=(0,) * 6, last_consumption_count=0,
                differential_consumption_intervals=(0,) * 53, transmit_time_offset=0):
        def many(values, count):
            assert len(values) == count
            return [b for v in values for b in _bits(int(v), 8)]
        return _bits(packet_type, 8) + _bits(packet_length, 16) + _bits(application_version, 8) + _bits(ert_type, 8) + _bits(ert_id, 32) + \
            _bits(consumption_interval_count, 8) + _bits(module_programming_state, 8) + many(tamper_count, 6) + many(async_count, 2) + \
            many(power_outage_flags, 6) + _bits(last_consumption_count, 32) + many(differential_consumption_intervals, 53) + \
            _bits(transmit_time_offset, 16) + _bits(idm_crc(_bits(ert_id, 32), 0, 32), 16)

    def random_fields(self, rng):
        return dict(application_version=int(rng.integers(256)), ert_type=int(rng.integers(256)), ert_id=int(rng.integers(1 << 32)),
                    consumption_interval_count=int(rng.integers(256)), module_programming_state=int(rng.integers(256)),
                    tamper_count=rng.integers(0, 256, 6).tolist(), async_count=rng.integers(0, 256, 2).tolist(),
                    power_outage_flags=rng.integers(0, 256, 6).tolist(), last_consumption_count=int(rng.integers(1 << 32)),
                    differential_consumption_intervals=rng.integers(0, 256, 53).tolist(), transmit_time_offset=int(rng.integers(1 << 16)))


def same_records(got, want):
    """equal field names, field types, shape and values.  (Neither tobytes() nor dtype equality: numpy drops the padding of padded records
    when it concatenates them.  What a block returns is checked with pads_are_zero and against the type's dtype where it is returned.)"""
    names = want.dtype.names
    return got.dtype.names == names and got.ndim == 1 and got.shape == want.shape and \
        all(got.dtype[k] == want.dtype[k] and np.array_equal(got[k], want[k]) for k in names)


def concat(parts, dtype):
    """np.concatenate that keeps the padded dtype"""
    out = np.zeros(sum(len(p) for p in parts), dtype)
    at = 0
    for p in parts:
        assert p.dtype == dtype
        out[at:at + len(p)] = p
        at += len(p)
    return out


def pads_are_zero(records):
    """the bytes of a structured array (as a block returned it, not a concatenation) that belong to no field"""
    dt = records.dtype
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(len(records), dt.itemsize)
    used = np.zeros(dt.itemsize, bool)
    for k in dt.names:
        used[dt.fields[k][1]:dt.fields[k][1] + dt.fields[k][0].itemsize] = True
    return not raw[:, ~used].any()


def _bits(value, n):
    return [(value >> (n - 1 - i)) & 1 for i in range(n)]


SCM = _SCM("scm", 96, 21, 0x1f2a60, 75, 0, _poly_rows(75, 0x6f63), types.SCMFrameType)
SCM_PLUS = _SCMPlus("scm+", 128, 16, 0x16a3, 112, 0x7b06, _poly_rows(112, 0x1021), types.SCMPlusFrameType)
IDM = _IDM("idm", 736, 32, 0x555516a3, 704, 0x866b, _idm_rows(), types.IDMFrameType)
PROTOCOLS = {"scm": SCM, "scm+": SCM_PLUS, "idm": IDM}


def encode_message(proto, msg):
    """the frame of the cw_len - 16 message bits `msg`: the preamble, the message - for IDM with its serial CRC field (frame bits 704 .. 719)
    set to the CRC of frame bits 72 .. 103 - and the check bits: the initial syndrome XOR the rows of the set message bits, because the last 16
    rows are the identity"""
    msg = [int(b) for b in msg]
    assert len(msg) == proto.cw_len - 16
    if proto is IDM:
        msg[672:688] = _bits(idm_crc(msg, 40, 32), 16)
    s = proto.init
    for i, b in enumerate(msg):
        if b:
            s ^= proto.rows[i]
    return np.array(list(proto.pre_bytes) + msg + _bits(s, 16), np.uint8)


def encode(proto, **fields):
    """(L bits, the record fields the framer reports for them)"""
    bits = encode_message(proto, proto.message(**fields))
    return bits, proto.fields(bytearray(bits.tobytes()))


def random_frame(proto, rng):
    return encode(proto, **proto.random_fields(rng))


class FramerLiteral:
    """process() of the three framers, buffer and in-place correction included"""

    def __init__(self, proto):
        self.proto, self.buf = proto, bytearray()

    def process(self, x):
        x = np.ascontiguousarray(x, np.uint8).tobytes()
        P, buf, out = self.proto, self.buf, []
        i, n = 0, len(x)
        while i < n:
            if len(buf) < P.L:
                k = min(P.L - len(buf), n - i)
                buf += x[i:i + k]
                i += k
            else:
                del buf[0]
                buf.append(x[i])
                i += 1
            if len(buf) == P.L:
                f = P.try_frame(buf)
                if f is not None:
                    out.append(f)
                    del buf[:]
        return P.records(out)


def pure_window_walk(proto, x):
    """every window judged on the raw bytes (a correction never outlives its window); L on after a frame, one on after a rejection"""
    x = np.ascontiguousarray(x, np.uint8).tobytes()
    out, s = [], 0
    while s + proto.L <= len(x):
        f = proto.try_frame(bytearray(x[s:s + proto.L]))
        if f is not None:
            out.append(f)
            s += proto.L
        else:
            s += 1
    return proto.records(out)


def uncorrectable_pair(proto, lo, hi):
    """two codeword indexes in [lo, hi) whose rows XOR to no row and not to zero"""
    for a in range(lo, hi):
        for b in range(a + 1, hi):
            s = proto.rows[a] ^ proto.rows[b]
            if s and s not in proto.correct:
                return a, b
    raise AssertionError("no such pair")


def persistent_case(proto, chain=1, seed=5):
    """(stream, fields): a valid frame with chain + 1 codeword bits flipped - any two of them uncorrectable - behind `chain` mutating windows at
    distance d = preamble + 16 from each other and from the frame: each is the preamble and 16 free bits, found by search so that the window, on
    the bytes the literal model holds when it gets there, has the syndrome of exactly one of the flipped bits and then fails its later check
    (protocol id / packet type, the first 8 free bits).  The literal model repairs the frame bit by bit and emits it; judged on the raw bytes
    the frame stays uncorrectable.  The frame starts at chain * d."""
    assert proto is not SCM, "an SCM window that corrects is accepted: it cannot leave a flip behind"
    d = proto.pre_bits + 16
    bits, want = random_frame(proto, np.random.default_rng(seed))
    # flipped codeword indexes, small so that every mutating window still covers its own; pairwise (and all together) uncorrectable
    base = 40
    while True:
        flips = [base + 7 * j for j in range(chain + 1)]
        ok = True
        for m in range(1 << len(flips)):
            s = 0
            for j, k in enumerate(flips):
                if (m >> j) & 1:
                    s ^= proto.rows[k]
            if bin(m).count("1") >= 2 and (s == 0 or s in proto.correct):
                ok = False
        if ok:
            break
        base += 1
    frame_at = chain * d
    stream = np.zeros(frame_at + proto.L, np.uint8)
    stream[frame_at:] = bits
    for k in flips:
        stream[frame_at + proto.cw_off + k] ^= 1
    bad = 0x1e if proto is SCM_PLUS else 0x1c
    for j in range(chain - 1, -1, -1):
        at = j * d
        stream[at:at + proto.pre_bits] = proto.preamble()
        # what the literal model holds when window j is tested: the flips of the windows before it are repaired
        held = stream.copy()
        for k in flips[:j]:
            held[frame_at + proto.cw_off + k] ^= 1
        target = frame_at + proto.cw_off + flips[j] - at - proto.cw_off              # codeword index of flip j in window j
        assert 16 <= target < proto.cw_len
        held[at + proto.pre_bits:at + d] = 0
        need = proto.syndrome(bytearray(held[at:at + proto.L].tobytes())) ^ proto.rows[target]
        found = None
        for v in range(1 << 16):
            if (v >> 8) == bad:
                continue
            s = 0
            for t in range(16):
                if (v >> (15 - t)) & 1:
                    s ^= proto.rows[t]
            if s == need:
                found = v
                break
        assert found is not None, "no free bits for window %d" % j
        stream[at + proto.pre_bits:at + d] = _bits(found, 16)
    return stream, want, flips


def _header(proto):
    """the message bits the protocol's later checks pin down (SCM+: protocol id; IDM: packet type and length)"""
    return {"scm": [], "scm+": _bits(0x1e, 8), "idm": _bits(0x1c, 8) + _bits(0x5cc6, 16)}[proto.name]


def overlap_stream(proto, d, rng):
    """(stream of d + L bits, fields of the first frame, fields of the second): two valid frames, the second starting d bits into the first.
    d = L - 1: the second's first bit is the first's last check bit, so first frames are drawn until that bit is the preamble's first.
    Otherwise (d at least 32 and behind the first's header; the second's preamble and header inside the first's message, before the first's
    check bits and IDM serial CRC): the first frame's message spells the second's preamble and header at d, and the second's remaining d bits - free message bits, for IDM its serial CRC, and its check bits - follow."""
    L, pre = proto.L, proto.pre_bits
    if d == L - 1:
        while True:
            first, _ = random_frame(proto, rng)
            if first[-1] == proto.pre_bytes[0]:
                break
        second, _ = random_frame(proto, rng)
        stream = np.concatenate([first, second[1:]])
    else:
        head = list(proto.pre_bytes) + _header(proto)
        assert max(pre + len(_header(proto)), 32) <= d and d + len(head) <= L - (32 if proto is IDM else 16)
        msg = rng.integers(0, 2, proto.cw_len - 16).tolist()
        msg[:len(_header(proto))] = _header(proto)
        msg[d - pre:d - pre + len(head)] = head
        first = encode_message(proto, msg)
        assert list(first[d:d + len(head)]) == head
        msg2 = list(first[d + pre:]) + rng.integers(0, 2, d).tolist()
        second = encode_message(proto, msg2[:proto.cw_len - 16])
        assert np.array_equal(second[:L - d], first[d:])
        stream = np.concatenate([first, second[L - d:]])
    a, b = proto.try_frame(bytearray(stream[:L].tobytes())), proto.try_frame(bytearray(stream[d:].tobytes()))
    assert a is not None and b is not None
    return stream, a, b


def golden_cases(name):
    """[(desc, bits, expected records)] of the reference's spec of one framer (tests/golden/make_golden_ert_framers.py)"""
    from tests import golden_util
    P = PROTOCOLS[name]
    doc = golden_util.load({"scm": "scmframer_spec", "scm+": "scmplusframer_spec", "idm": "idmframer_spec"}[name])
    assert len(doc["vectors"]) == 6
    return [(v["desc"], np.asarray(v["inputs"][0], np.uint8), P.records([dict(zip(P.golden_order, f)) for f in v["outputs"][0]["frames"]]))
            for v in doc["vectors"]]
