"""BinaryPhaseCorrectorBlock's CPU models (tests/helpers/phasecorr_model.py): the reference's golden vectors, the drift of the reference's
running sum from the window mean, and the device's fixed-point window sums against the f64 mean."""
import numpy as np
import pytest

from tests import golden_util
from tests.helpers import phasecorr_model as pm


@pytest.mark.parametrize("form", ["lua", "mean", "mean_fast", "fixed"])
def test_models_reproduce_golden(form):
    doc = golden_util.load("binaryphasecorrector_spec")
    assert len(doc["vectors"]) == 4
    for v in doc["vectors"]:
        N, I = v["args"]
        got = pm.correct(v["inputs"][0], N, I, form)
        assert golden_util.max_abs_err(got, v["outputs"][0]) <= doc["epsilon"]


def test_lua_running_sum_drifts_from_window_mean():
    """the reference subtracts the Float32-rounded evicted phase from a double sum: a random walk of ~ulp_f32(phi) / (2N) per measurement.
    Within 1e-6 of the window mean for 2^14 measurements; after 2^20 it has wandered ~10x further (sqrt(64) = 8)."""
    rng = np.random.default_rng(1)
    phi = rng.uniform(-1.5, 1.5, 1 << 20)
    d = np.abs(pm.lua_average(phi, 50) - pm.window_mean_fast(phi, 50))
    short, long_ = d[:1 << 14].max(), d.max()
    assert short < 1e-6
    assert long_ > 4 * short and 1e-7 < long_ < 1e-5


@pytest.mark.parametrize("N", [1, 4, 50, 3000, 8000])
def test_fixed_point_equals_f64_mean(N):
    rng = np.random.default_rng(N)
    phi = pm.phases((rng.standard_normal(6000) + 1j * rng.standard_normal(6000)).astype(np.complex64), 1)
    assert np.max(np.abs(pm.fixed_average(phi, N) - pm.window_mean(phi, N))) < 1e-12


def test_quant_shift_bounds_window_sums():
    """any window sum of N quantised phases |q| <= 2^(s+1) stays within 62 bits"""
    for N in [1, 2, 3, 50, 3000, 8000, 1 << 20, (1 << 24) - 1, 1 << 24]:
        s = pm.quant_shift(N)
        assert N * 2 ** (s + 1) <= 2 ** 62 and s >= 36


def test_nan_is_sticky():
    x = np.ones(40, np.complex64)
    x[9] = np.nan
    y = pm.correct(x, 4, 3, "fixed")
    assert not np.isnan(y[:9]).any() and np.isnan(y[9:]).all()
    y = pm.correct(x, 4, 2, "fixed")                # sample 9 is not measured: only it is NaN
    assert np.isnan(y).tolist() == [i == 9 for i in range(40)]
