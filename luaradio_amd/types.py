"""Sample types - mirrors radio/types/complexfloat32.lua:19-24 and radio/types/float32.lua:17-21.

ComplexFloat32 = struct{float real, imag} (8 B interleaved) == numpy complex64;
Float32 = struct{float value} (4 B) == numpy float32; Bit = struct{uint8_t value} (1 B) == numpy uint8; RDSFrameType = struct{uint16_t blocks[4]} (8 B) == a
row of four numpy uint16; SCMFrameType (16 B), SCMPlusFrameType (16 B) and IDMFrameType (88 B) == numpy structured dtypes of the records in
include/lrhip.h.  Vectors are contiguous numpy arrays, which is the
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
