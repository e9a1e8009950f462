"""Sample types - mirrors radio/types/complexfloat32.lua:19-24 and radio/types/float32.lua:17-21.

ComplexFloat32 = struct{float real, imag} (8 B interleaved) == numpy complex64;
Float32 = struct{float value} (4 B) == numpy float32; Bit = struct{uint8_t value} (1 B) and Byte = struct{uint8_t value} (1 B) == numpy uint8; RDSFrameType = struct{uint16_t blocks[4]} (8 B) == a
row of four numpy uint16; SCMFrameType (16 B), SCMPlusFrameType (16 B) and IDMFrameType (88 B), AX25FrameType (416 B) and POCSAGFrameType (256 B) == numpy structured
dtypes of the records in include/lrhip.h.  Vectors are contiguous numpy arrays, which is the
same raw layout the reference writes on its pipes (radio/types/cstruct.lua:87-126).
"""
import numpy as np


class _SampleType:
    def __init__(self, name, dtype, size):
        self.name, self.dtype, self.size = name, np.dtype(dtype), size

    def vector(self, n=0):
        return np.zeros(n, dtype=self.dtype)

    def vector_from_array(self, arr):
        if self.dtype == np.complex64:
            a = np.asarray(arr, dtype=np.float64)
            if a.ndim == 2:       # {{re, im}, ...} as in the reference
                return (a[:, 0] + 1j * a[:, 1]).astype(np.complex64)
            return np.asarray(arr).astype(np.complex64)
        if self.dtype == np.uint8:
            return np.asarray(arr).astype(np.uint8)
        return np.asarray(arr, dtype=np.float64).astype(np.float32)

    def __repr__(self):
        return self.name


ComplexFloat32 = _SampleType("ComplexFloat32", np.complex64, 8)
Float32 = _SampleType("Float32", np.float32, 4)
# radio/types/bit.lua: struct bit {uint8_t value} (1 B)
Bit = _SampleType("Bit", np.uint8, 1)
# radio/types/byte.lua: struct byte {uint8_t value} (1 B); the same raw layout as Bit, so type_of(uint8) keeps answering Bit
Byte = _SampleType("Byte", np.uint8, 1)
# radio/blocks/protocol/rdsframer.lua:71-75: rds_frame_t {uint16_t blocks[4]} (8 B); a vector of n frames is an (n, 4) uint16 array
RDSFrameType = _SampleType("RDSFrameType", np.dtype((np.uint16, (4,))), 8)


def _record(fields, itemsize):
    """structured dtype with explicit offsets: [(name, format, offset)]"""
    return np.dtype({"names": [f[0] for f in fields], "formats": [f[1] for f in fields], "offsets": [f[2] for f in fields], "itemsize": itemsize})


# radio/blocks/protocol/scmframer.lua:103-114, scmplusframer.lua:119-129, idmframer.lua:76-95: the reference's frame objects as fixed little-endian
# records (include/lrhip.h), with the reference's field names; the pad bytes are zero and not part of the dtype
SCMFrameType = _SampleType("SCMFrameType", _record([
    ("ert_id", "<u4", 0), ("consumption", "<u4", 4), ("crc", "<u2", 8), ("ert_type", "u1", 10), ("physical_tamper", "u1", 11),
    ("encoder_tamper", "u1", 12), ("reserved", "u1", 13)], 16), 16)
SCMPlusFrameType = _SampleType("SCMPlusFrameType", _record([
    ("ert_id", "<u4", 0), ("consumption", "<u4", 4), ("tamper", "<u2", 8), ("crc", "<u2", 10), ("protocol_id", "u1", 12), ("ert_type", "u1", 13)], 16), 16)
IDMFrameType = _SampleType("IDMFrameType", _record([
    ("ert_id", "<u4", 0), ("last_consumption_count", "<u4", 4), ("transmit_time_offset", "<u2", 8), ("serial_crc", "<u2", 10),
    ("packet_crc", "<u2", 12), ("application_version", "u1", 14), ("ert_type", "u1", 15), ("consumption_interval_count", "u1", 16),
    ("module_programming_state", "u1", 17), ("tamper_count", ("u1", (6,)), 18), ("async_count", ("u1", (2,)), 24),
    ("power_outage_flags", ("u1", (6,)), 26), ("differential_consumption_intervals", ("u1", (53,)), 32)], 88), 88)


# radio/blocks/protocol/ax25framer.lua:55-64 and pocsagframer.lua:82-90: the reference's frames are Lua objects of variable length; on the device
# they are fixed little-endian records (struct lrhip_ax25_frame, struct lrhip_pocsag_frame in include/lrhip.h) and frames() gives the objects back
class _AX25FrameType(_SampleType):
    def frames(self, records):
        """the reference's objects: [{"addresses": [{"callsign": bytes(6), "ssid": int}, ...], "control", "pid" (None when absent),
        "payload" (bytes, or None when absent)}, ...]"""
        out = []
        for r in np.asarray(records, self.dtype):
            data = r["data"].tobytes()
            addresses = [{"callsign": bytes(b >> 1 for b in data[7 * k:7 * k + 6]), "ssid": data[7 * k + 6] >> 1} for k in range(int(r["num_addresses"]))]
            has_pid = bool(r["has_pid"])
            at = int(r["payload_offset"])
            out.append({"addresses": addresses, "control": int(r["control"]), "pid": int(r["pid"]) if has_pid else None,
                        "payload": data[at:at + int(r["payload_length"])] if has_pid else None})
        return out


class _POCSAGFrameType(_SampleType):
    CONTINUES, CONTINUED = 1, 2                 # flags: this frame continues in the next record / this record continues the previous one

    def frames(self, records):
        """the reference's objects, continuation records merged: [{"address", "func", "data": [word, ...]}, ...]"""
        out = []
        for r in np.asarray(records, self.dtype):
            words = [int(w) for w in r["data"][:int(r["count"])]]
            if int(r["flags"]) & self.CONTINUED and out:
                out[-1]["data"].extend(words)
            else:
                out.append({"address": int(r["address"]), "func": int(r["func"]), "data": words})
        return out


AX25FrameType = _AX25FrameType("AX25FrameType", _record([
    ("length", "<u2", 0), ("crc", "<u2", 2), ("num_addresses", "u1", 4), ("control", "u1", 5), ("pid", "u1", 6), ("has_pid", "u1", 7),
    ("payload_offset", "<u2", 8), ("payload_length", "<u2", 10), ("data", ("u1", (400,)), 16)], 416), 416)
POCSAGFrameType = _POCSAGFrameType("POCSAGFrameType", _record([
    ("address", "<u4", 0), ("func", "u1", 4), ("flags", "u1", 5), ("count", "<u2", 6), ("data", ("<u4", (62,)), 8)], 256), 256)


def type_of(x):
    """data_type of a vector (numpy array)."""
    x = np.asarray(x)
    if x.dtype == np.complex64:
        return ComplexFloat32
    if x.dtype == np.float32:
        return Float32
    if x.dtype == np.uint8:
        return Bit
    raise TypeError("Unsupported sample dtype %s (expected complex64, float32 or uint8)" % x.dtype)
