"""Loader for the reference golden vectors committed under tests/golden/ (see make_golden.py)."""
import gzip
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _vec(v):
    """{"type","data"} -> numpy array (complex64 / float32); anything else is returned unchanged."""
    if isinstance(v, dict) and "data" in v:
        if v["type"] == "ComplexFloat32":
            a = np.array(v["data"], dtype=np.float64).reshape(-1, 2)
            return (a[:, 0] + 1j * a[:, 1]).astype(np.complex64)
        if v["type"] == "Float32":
            return np.array(v["data"], dtype=np.float64).astype(np.float32)
        return np.array(v["data"])
    if isinstance(v, dict) and "scalar" in v:
        if v["type"] == "ComplexFloat32":
            return np.complex64(complex(v["scalar"][0], v["scalar"][1]))
        return np.float32(v["scalar"][0])
    if isinstance(v, dict) and v.get("type") == "bytes":
        return bytes.fromhex(v["hex"])
    return v


def load(name):
    with gzip.open(os.path.join(GOLDEN_DIR, name + ".json.gz")) as f:
        doc = json.load(f)
    if doc["kind"] == "block":
        eps = doc["epsilon"]
        # composite epsilons are Lua expressions "(liquid and not volk) and 1e-3 or 1e-5": take the non-liquid value
        doc["epsilon"] = float(eps.split(" or ")[-1]) if " or " in eps else float(eps)
        for v in doc["vectors"]:
            v["args"] = [_vec(a) for a in v["args"]]
            v["inputs"] = [_vec(a) for a in v["inputs"]]
            v["outputs"] = [_vec(a) for a in v["outputs"]]
    else:
        doc["values"] = {k: _vec(v) for k, v in doc["values"].items()}
    return doc


def max_abs_err(a, b):
    """jigs.assert_vector_equal metric: |x-y| per sample (complex modulus for ComplexFloat32)."""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a.astype(np.complex128) - b.astype(np.complex128))))


def run_whole_and_samplewise(make_block, x):
    """The two modes of tests/jigs.lua:191-250: whole vector in one process() call, and one sample per call."""
    whole = make_block().process(x)
    blk = make_block()
    parts = [blk.process(x[i:i + 1]) for i in range(len(x))]
    parts = [p for p in parts if len(p)]
    samplewise = np.concatenate(parts) if parts else whole[:0]
    return whole, samplewise


def pack_edge_values():
    """Float32 samples at the edges of the file-sink record conversion (lro_format_pack / format_pack_kernel): exact +-1 and 0, -0.0,
    one ulp inside +-1, subnormals, |x| in (1, 4], magnitudes past every integer type's range, NaN and +-inf"""
    sub = np.array([1, 2, 0x7fffff, 0x400000], np.uint32).view(np.float32)
    e = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1 - 2.0 ** -24, -1 + 2.0 ** -24, 2.0 ** -24, -2.0 ** -24, 1 / 127.5, -1 / 127.5,
         1.0000001, -1.0000001, 1.5, -1.5, 2.0, -2.0, 3.999, -3.999, 4.0, -4.0, 255.0, -255.0, 1e3, -1e3, 65536.5, -65536.5,
         2.0 ** 31, -2.0 ** 31, 2.0 ** 32, 1e10, -1e10, 2.0 ** 62, 2.0 ** 63, -2.0 ** 63, 2.0 ** 64, 3.4e38, -3.4e38,
         np.nan, np.inf, -np.inf]
    return np.concatenate([np.array(e, np.float32), sub, -sub])


def u32_pack_straddle():
    """tests/golden/u32_pack_straddle.json: the float32 inputs in [-1, 1] whose u32 record differs between two roundings and one"""
    with open(os.path.join(GOLDEN_DIR, "u32_pack_straddle.json")) as f:
        doc = json.load(f)
    return np.array([int(b, 16) for b in doc["bits"]], np.uint32).view(np.float32), doc["two_roundings"], doc["one_rounding"]
