"""AX25FramerBlock (radio/blocks/protocol/ax25framer.lua:94-284) in Python: the literal transcription of its process() loop, the packing of its
frames into types.AX25FrameType records (include/lrhip.h), a frame builder (FCS, bit stuffing, flags) and the hop formulation the device
kernels implement (luaradio_amd/csrc/kernels_ax25framer.h).  Bytes are read as the reference reads them: Bit.tonumber counts a byte as 1 only
when it equals 1, the unstuffer drops a byte only when it equals 0, and the CRC feeds back only when (crc & 1) ^ value == 1."""
import numpy as np

from luaradio_amd import types

RAW_MAXLEN = 3184            # AX25_RAW_FRAME_MAXLEN: a raw frame of 3185 bits still closes, one of 3186 does not
FRAME_MINLEN = 136           # AX25_FRAME_MINLEN
FLAG = 0x7e
FLAG_BITS = np.array([0, 1, 1, 1, 1, 1, 1, 0], np.uint8)
DTYPE = types.AX25FrameType.dtype
IDLE, FRAME = 1, 2


def tonumber_lsb(buf, offset, length):
    v = 0
    for i in range(length):
        if buf[offset + i] == 1:
            v |= 1 << i
    return v


def compute_crc(bits, length):
    """ax25_compute_crc (:94-111) on byte values"""
    crc = 0xffff
    for i in range(length):
        if ((crc & 1) ^ int(bits[i])) == 1:
            crc = (crc >> 1) ^ 0x8408
        else:
            crc >>= 1
    return ~crc & 0xffff


def unstuff(raw):
    """ax25_unstuff_frame (:113-133)"""
    out, ones = [], 0
    for v in raw:
        if not (ones == 5 and v == 0):
            out.append(v)
        ones = ones + 1 if v == 1 else 0
    return out


def validate(frame):
    """ax25_validate_frame (:135-154)"""
    n = len(frame)
    if n % 8 != 0 or n + 16 < FRAME_MINLEN:
        return False
    return compute_crc(frame, n - 16) == tonumber_lsb(frame, n - 16, 16)


def extract(frame):
    """ax25_extract_frame (:156-216): the frame as a dict with the reference's fields plus the octets and the FCS, or None"""
    n, at = len(frame), 0
    addresses = []
    while True:
        callsign = b""
        for _ in range(6):
            if at >= n - 16:
                return None
            callsign += bytes([tonumber_lsb(frame, at, 8) >> 1])
            at += 8
        if at >= n - 16:
            return None
        byte = tonumber_lsb(frame, at, 8)
        at += 8
        addresses.append({"callsign": callsign, "ssid": byte >> 1})
        if byte & 1:
            break
    if at >= n - 16:
        return None
    control = tonumber_lsb(frame, at, 8)
    at += 8
    pid = payload = None
    offset = at // 8
    if at < n - 16:
        pid = tonumber_lsb(frame, at, 8)
        at += 8
        offset = at // 8
        payload = bytes(tonumber_lsb(frame, k, 8) for k in range(at, n - 16, 8))
    return {"addresses": addresses, "control": control, "pid": pid, "payload": payload, "payload_offset": offset,
            "crc": tonumber_lsb(frame, n - 16, 16), "octets": bytes(tonumber_lsb(frame, k, 8) for k in range(0, n - 16, 8))}


def evaluate(raw):
    """a closed raw frame -> its frame, or None (:249-252)"""
    frame = unstuff(raw)
    return extract(frame) if validate(frame) else None


def objects(frames):
    """what types.AX25FrameType.frames() returns for these frames"""
    return [{k: f[k] for k in ("addresses", "control", "pid", "payload")} for f in frames]


def records(frames):
    out = np.zeros(len(frames), DTYPE)
    for r, f in zip(out, frames):
        has_pid = f["pid"] is not None
        r["length"], r["crc"], r["num_addresses"], r["control"] = len(f["octets"]), f["crc"], len(f["addresses"]), f["control"]
        r["pid"], r["has_pid"] = (f["pid"], 1) if has_pid else (0, 0)
        r["payload_offset"], r["payload_length"] = f["payload_offset"], len(f["payload"]) if has_pid else 0
        r["data"][:len(f["octets"])] = np.frombuffer(f["octets"], np.uint8)
    return out


def same_records(got, want):
    """equal field names, field types, shape and values (numpy drops the padding of padded records when it concatenates them, so neither
    tobytes() nor dtype equality)"""
    names = want.dtype.names
    return got.dtype.names == names and got.ndim == 1 and got.shape == want.shape and \
        all(got.dtype[k] == want.dtype[k] and np.array_equal(got[k], want[k]) for k in names)


def pads_are_zero(rec):
    """the bytes that belong to no field, and the tail of `data` behind `length`"""
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), DTYPE.itemsize)
    return not raw[:, 12:16].any() and all(not r["data"][int(r["length"]):].any() for r in rec)


def concat(parts):
    out = np.zeros(sum(len(p) for p in parts), DTYPE)
    at = 0
    for p in parts:
        assert p.dtype == DTYPE
        out[at:at + len(p)] = p
        at += len(p)
    return out


class FramerLiteral:
    """process() of ax25framer.lua:218-284, statement by statement"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.state, self.buf, self.raw = IDLE, [], []

    def process_frames(self, x):
        out, i, n = [], 0, len(x)
        x = [int(v) for v in np.asarray(x, np.uint8)]
        while i < n:
            if len(self.buf) < 8:
                k = min(8 - len(self.buf), n - i)
                self.buf.extend(x[i:i + k])
                i += k
            if len(self.buf) != 8:
                continue
            is_flag = tonumber_lsb(self.buf, 0, 8) == FLAG
            if self.state == IDLE:
                if is_flag:
                    self.raw, self.buf, self.state = [], [], FRAME
                else:
                    del self.buf[0]
            elif is_flag:
                frame = evaluate(self.raw)
                if frame is not None:
                    out.append(frame)
                    self.buf, self.state = [], IDLE
                else:
                    self.raw, self.buf = [], []
            elif len(self.raw) > RAW_MAXLEN:
                self.state = IDLE
            else:
                self.raw.append(self.buf.pop(0))
        return out

    def process(self, x):
        return records(self.process_frames(x))


def hop_frames(x):
    """The hop formulation, on a whole stream: the consumed flags are the greedy chain "first flag at or after q, then q = p + 8"; a segment
    between two consecutive consumed flags is a candidate unless the segment before it was emitted; a candidate of at most 3185 raw bits is
    emitted when it evaluates."""
    x = np.asarray(x, np.uint8)
    n = len(x)
    ones = (x == 1)
    is_flag = np.zeros(max(n - 7, 0), bool)
    if n >= 8:
        is_flag[:] = True
        for k in range(8):
            is_flag &= ones[k:n - 7 + k] == bool(FLAG_BITS[k])
    where = np.flatnonzero(is_flag)
    flags, q = [], 0
    while True:
        k = int(np.searchsorted(where, q))
        if k == len(where):
            break
        flags.append(int(where[k]))
        q = flags[-1] + 8
    out, emitted = [], False
    for a, b in zip(flags[:-1], flags[1:]):
        frame = None
        if not emitted and b - (a + 8) <= RAW_MAXLEN + 1:
            frame = evaluate([int(v) for v in x[a + 8:b]])
        emitted = frame is not None
        if emitted:
            out.append(frame)
    return out


# ---- building frames
def octets_of(addresses, control, pid=None, payload=b""):
    """addresses: [(callsign of 6 bytes, ssid of 7 bits)]; the last carries the end-of-address bit"""
    out = bytearray()
    for k, (callsign, ssid) in enumerate(addresses):
        assert len(callsign) == 6
        out += bytes(c << 1 for c in callsign)
        out.append((ssid << 1) | (1 if k == len(addresses) - 1 else 0))
    out.append(control)
    if pid is not None:
        out.append(pid)
        out += payload
    return bytes(out)


def bits_of(octets):
    return np.unpackbits(np.frombuffer(bytes(octets), np.uint8), bitorder="little") if len(octets) else np.zeros(0, np.uint8)


def with_fcs(octets):
    """the unstuffed frame bits: the octets LSB first, then the 16 FCS bits"""
    bits = bits_of(octets)
    crc = compute_crc(bits, len(bits))
    return np.concatenate([bits, np.array([(crc >> k) & 1 for k in range(16)], np.uint8)])


def stuff(bits):
    out, ones = [], 0
    for v in bits:
        out.append(int(v))
        ones = ones + 1 if v == 1 else 0
        if ones == 5:
            out.append(0)
            ones = 0
    return np.array(out, np.uint8)


def raw_of(octets):
    """the stuffed bits between the flags"""
    return stuff(with_fcs(octets))


def framed(octets, opening=1, closing=1):
    return np.concatenate([np.tile(FLAG_BITS, opening), raw_of(octets), np.tile(FLAG_BITS, closing)])


def frame_of(octets):
    """the frame the framer extracts from these octets (None when it does not extract)"""
    return extract([int(v) for v in with_fcs(octets)])


def random_octets(rng, payload_len=None, naddr=None, pid=True):
    naddr = int(rng.integers(1, 4)) if naddr is None else naddr
    addresses = [(bytes(int(v) for v in rng.integers(32, 91, 6)), int(rng.integers(0, 128))) for _ in range(naddr)]
    payload_len = int(rng.integers(0, 40)) if payload_len is None else payload_len
    # at least 13 octets with the addresses: pad the payload of a short frame
    need = max(0, 13 - (7 * naddr + 2))
    payload_len = max(payload_len, need) if pid else 0
    return octets_of(addresses, int(rng.integers(0, 256)), int(rng.integers(0, 256)) if pid else None, bytes(int(v) for v in rng.integers(0, 256, payload_len)))


def minimal_octets(seed=15):
    """13 octets whose raw frame needs no stuffed bit: 136 bits with its two flags (searched; deterministic)"""
    rng = np.random.default_rng(seed)
    while True:
        octets = random_octets(rng, naddr=1, payload_len=4)
        if len(octets) == 13 and len(raw_of(octets)) == 120:
            return octets


def long_octets(length, stuffed):
    """`length` octets whose raw frame has exactly `stuffed` stuffed bits (searched; deterministic)"""
    rng = np.random.default_rng(100 + stuffed)
    while True:
        octets = bytes([0x40] * 6 + [0x41, 0x03, 0xf0]) + bytes(int(v) for v in rng.choice([0x00, 0x11, 0x24, 0x49, 0x52], length - 9))
        for k in range(stuffed):
            octets = octets[:20 + 2 * k] + b"\x1f" + octets[21 + 2 * k:]
        if len(raw_of(octets)) == 8 * length + 16 + stuffed:
            return octets


def random_stream(rng, pieces=12):
    """noise, flag runs, valid frames, a frame with one flipped bit followed by a valid one, frames sharing a flag, 0111111 in front of a flag"""
    parts = []
    for _ in range(pieces):
        kind = int(rng.integers(0, 7))
        if kind == 0:
            parts.append(rng.integers(0, 2, int(rng.integers(1, 300))).astype(np.uint8))
        elif kind == 1:
            parts.append(np.tile(FLAG_BITS, int(rng.integers(1, 6))))
        elif kind == 2:
            parts.append(framed(random_octets(rng), int(rng.integers(1, 3)), int(rng.integers(1, 3))))
        elif kind == 3:
            bad = framed(random_octets(rng), 1, 0)
            bad[8 + int(rng.integers(0, len(bad) - 8))] ^= 1
            parts.append(np.concatenate([bad, framed(random_octets(rng))]))
        elif kind == 4:
            parts.append(np.concatenate([framed(random_octets(rng), 1, 0)] + [framed(random_octets(rng), 1, 0) for _ in range(int(rng.integers(1, 3)))]
                                        + [FLAG_BITS]))
        elif kind == 5:
            parts.append(np.concatenate([np.array([0, 1, 1, 1, 1, 1, 1], np.uint8), framed(random_octets(rng))]))
        else:
            parts.append(np.concatenate([framed(random_octets(rng, pid=bool(rng.integers(0, 2)))), rng.integers(0, 2, int(rng.integers(0, 20))).astype(np.uint8)]))
    return np.concatenate(parts)


def golden_cases():
    """[(desc, bits, expected frames as types.AX25FrameType.frames() gives them)] of the reference's spec
    (tests/golden/make_golden_packet_framers.py)"""
    from tests import golden_util
    doc = golden_util.load("ax25framer_spec")
    assert len(doc["vectors"]) == 5
    return [(v["desc"], np.asarray(v["inputs"][0], np.uint8),
             [{"addresses": [{"callsign": a["callsign"].encode("latin-1"), "ssid": a["ssid"]} for a in addresses], "control": control, "pid": pid,
               "payload": payload.encode("latin-1")} for addresses, control, pid, payload in v["outputs"][0]["frames"]]) for v in doc["vectors"]]
