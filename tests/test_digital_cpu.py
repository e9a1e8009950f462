"""CPU side of the clock recovery / sampler / slicer / differential decoder: the golden vectors, the Python models, the clock recovery's closed
form against the literal loop, and the op strings that carry their double parameters."""
import ctypes as C

import numpy as np
import pytest

from luaradio_amd import _lib
from luaradio_amd.blocks import digital_op
from tests import golden_util
from tests.helpers import digital_model as dm

RATE = 2.0          # the reference jig's rate (tests/jigs.lua)


def _bits(v):
    return np.asarray(v, np.uint8)


@pytest.mark.parametrize("name", ["zerocrossingclockrecovery_spec", "sampler_spec", "slicer_spec", "differentialdecoder_spec"])
def test_fixture_loads(name):
    doc = golden_util.load(name)
    assert doc["kind"] == "block" and len(doc["vectors"]) >= 2
    for v in doc["vectors"]:
        assert len(v["inputs"]) >= 1 and len(v["outputs"]) == 1


def test_models_reproduce_zerocrossingclockrecovery_fixture():
    for v in golden_util.load("zerocrossingclockrecovery_spec")["vectors"]:
        baud, thr = v["args"]
        P = RATE / baud
        x, want = v["inputs"][0], v["outputs"][0]
        assert np.array_equal(dm.ZcLiteral(P, thr).process(x), want)
        assert np.array_equal(dm.ZcFast(P, thr).process(x), want)
        zc = dm.ZcFast(P, thr)
        assert np.array_equal(np.concatenate([zc.process(x[i:i + 1]) for i in range(len(x))]), want)


def test_models_reproduce_sampler_fixture():
    for v in golden_util.load("sampler_spec")["vectors"]:
        data, clock = v["inputs"]
        want = v["outputs"][0]
        assert np.array_equal(dm.SamplerModel().process(data, clock), want)
        assert np.array_equal(dm.SamplerFast().process(data, clock), want)


def test_models_reproduce_slicer_fixture():
    for v in golden_util.load("slicer_spec")["vectors"]:
        assert np.array_equal(dm.slicer(v["inputs"][0], v["args"][0] if v["args"] else 0.0), _bits(v["outputs"][0]))


def test_models_reproduce_differentialdecoder_fixture():
    for v in golden_util.load("differentialdecoder_spec")["vectors"]:
        m = dm.DiffDecModel(v["args"][0])
        assert np.array_equal(m.process(_bits(v["inputs"][0])), _bits(v["outputs"][0]))


def test_differential_decoder_model_any_byte():
    x = np.arange(256, dtype=np.uint8)
    out = dm.DiffDecModel(True).process(x)
    prev = np.concatenate([[0], x[:-1]]).astype(int)
    assert np.array_equal(out, ((prev ^ x) + 1) % 2)


PERIODS = [2.0 / 0.4444, 12500 / 1200, 12500 / 512, 4.0, 7.999999, 1102500 / 1200]


def _stretches(n, seed):
    """noise with crossing-free stretches (DC runs) of up to 50 000 samples"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    pos = 0
    while pos < n:
        L = int(rng.integers(1, 50000))
        if rng.random() < 0.3:
            x[pos:pos + L] = np.float32(rng.choice([0.5, -0.5, 0.0]))
        pos += L + int(rng.integers(1, 20000))
    return x


@pytest.mark.parametrize("P", [P for P in PERIODS if dm.zc_closed_params(P) is not None])
def test_closed_form_equals_literal_loop(P):
    x = _stretches(10 ** 6, int(P * 1000) % 2 ** 31)
    lit = dm.ZcLiteral(P).process(x)
    fast = dm.ZcFast(P)
    assert fast.params is not None
    got = np.concatenate([fast.process(x[:333333]), fast.process(x[333333:700001]), fast.process(x[700001:])])
    assert np.array_equal(got, lit)


def test_closed_form_domain():
    assert dm.zc_closed_params(2.0 / 0.4444) is not None
    assert dm.zc_closed_params(12500 / 1200) is not None
    assert dm.zc_closed_params(4.0) is not None
    assert dm.zc_closed_params(7.999999) is None          # P + 1 crosses a power of two: every "+ P" may round
    assert dm.zc_closed_params(1.5) is None               # P < 2


def test_op_values_round_trip():
    vals = [12500 / 1200, 2.0 / 0.4444, 0.1, 1e-300, 123456789.123456789, -0.0, 5e-324]
    for v in vals:
        assert float("%.17g" % v) == v                     # the Lua glue's string.format
        assert float(repr(v)) == v
    assert digital_op("slicer", threshold=0.25) == "slicer:threshold=0.25"


@pytest.mark.parametrize("op", [
    "zerocrossingclockrecovery:period", "zerocrossingclockrecovery:period=", "zerocrossingclockrecovery:period=1.5x:threshold=0",
    "zerocrossingclockrecovery:=3", "zerocrossingclockrecovery:period=10:bogus=1", "slicer:threshold=1:threshold=2",
    "slicer:threshold=1e999", "absolutevalue:threshold=0", "nosuchblock:threshold=0", "differentialdecoder:invert=",
    "slicer:threshold=0:period=5", "differentialdecoder:invert=1:threshold=3", "clocksampler:period=10:threshold=0:invert=1",
])
def test_op_string_rejected(op):
    L = _lib.load()
    assert not L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    msg = L.lrhip_strerror().decode()
    assert msg and ("malformed" in msg or "unknown" in msg or "bad value" in msg or "twice" in msg), msg


@pytest.mark.parametrize("P", [7.999999, 12500 / 400, 48000 / 14400, 1.5, 1.0 + 2.0 ** -30])
def test_fallback_walk_equals_literal_loop(P):
    """periods without the closed form: the device's whole-symbol jumps, with the offset carried across calls and tiles, give the literal loop"""
    assert dm.zc_closed_params(P) is None
    x = _stretches(300000, 7)
    x[100000:250000] = 0.0                                  # never decisive at threshold 0: a crossing-free stretch many calls long
    lit = dm.ZcLiteral(P).process(x)
    jm = dm.ZcJump(P)
    edges = [0, 17, 4096, 50001, 100003, 140000, 180000, 220000, 260000, 300000]
    got = np.concatenate([jm.process(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    assert np.array_equal(got, lit)
