"""The decimal rounding of the device submission rows (mesm_windows_rows, postprocess.device_rows), emulated in numpy
(postprocess.round4_emulated: rint(double(x) * 1e4) / 1e4), against what the reference does with every number it
emits: float(f"{x:.4f}") of a float32 value (eval.py:74-78, utils/post_processing.py:22-47)."""
import math

import numpy as np


def _python(a):
    return np.array([float("%.4f" % float(x)) for x in np.asarray(a, dtype=np.float32).astype(np.float64)])


def _same(got, want):
    assert np.array_equal(got, want), (got[got != want][:5], want[got != want][:5])
    assert np.array_equal(np.signbit(got), np.signbit(want))


def test_dense_sweep_matches_python_formatting():
    from mesm_amd.postprocess import round4_emulated
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-300, 300, 200_000), rng.uniform(-1, 1, 100_000),
                        np.linspace(-300, 300, 100_001)]).astype(np.float32)
    _same(round4_emulated(x), _python(x))


def test_exact_decimal_ties_round_half_to_even():
    from mesm_amd.postprocess import round4_emulated
    k = np.arange(-312 * 32, 312 * 32 + 1)
    x = (k / 32.0).astype(np.float32)  # exact in float32; the odd k are decimal ties at the 5th digit (x.xxxx5)
    _same(round4_emulated(x), _python(x))
    assert round4_emulated(np.float32(0.03125)) == 0.0312 == float("%.4f" % 0.03125)
    assert round4_emulated(np.float32(0.09375)) == 0.0938


def test_negative_values_that_round_to_negative_zero():
    from mesm_amd.postprocess import round4_emulated
    x = np.array([-0.0, -1e-9, -0.00001, -0.00004, -0.00005, -4.9e-5], dtype=np.float32)
    got = round4_emulated(x)
    _same(got, _python(x))
    assert all(v == 0.0 and math.copysign(1.0, v) < 0 for v in got)
