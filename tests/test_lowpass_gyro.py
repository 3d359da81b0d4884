"""gfw_lowpass_gyro (Lowpass::filter_gyro_forward_backward, filtering.rs:46-74: biquad's second-order Butterworth low-pass in transposed direct form II, forward then
backward) against the statement's pure-Python loop (tests/_syncgyrostmt.py) — to the bit: both sides call the same libm for the one sin and cos — and, where
scipy is installed, against scipy.signal.lfilter run forward and then backward with the same coefficients.  Host only: no GPU."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, warp
import _syncgyrostmt as G


def series(n, seed=1):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 200.0
    return np.stack([30.0 * np.sin(2 * np.pi * 1.3 * t + k) + rng.normal(0.0, 4.0, n) for k in range(3)], axis=1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("freq,rate", [(20.0, 200.0), (20.0, 59.94), (20.0, 50.0), (20.0, 40.0), (20.0, 1963.7), (3.5, 120.0)])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 257])
def test_equals_the_statement_to_the_bit(freq, rate, n):
    x = series(n)
    got, applied = warp.lowpass_gyro(freq, rate, x)
    want, want_applied = G.lowpass_gyro(freq, rate, x)
    assert applied and want_applied
    assert same_bits(got, want)
    if n > 2:
        assert not same_bits(got, x)


def test_entries_without_a_gyro_are_skipped_and_do_not_advance_the_state():
    x = series(300, seed=2)
    has = np.ones(300, dtype=np.uint8)
    has[[0, 5, 6, 7, 150, 298, 299]] = 0
    got, applied = warp.lowpass_gyro(20.0, 200.0, x, has)
    assert applied and same_bits(got, G.lowpass_gyro(20.0, 200.0, x, has)[0])
    assert same_bits(got[has == 0], x[has == 0])                                      # untouched
    packed, _ = warp.lowpass_gyro(20.0, 200.0, x[has == 1])                           # the series without the gaps: the same filter run
    assert same_bits(got[has == 1], packed)
    none, _ = warp.lowpass_gyro(20.0, 200.0, x, np.zeros(300, dtype=np.uint8))
    assert same_bits(none, x)


@pytest.mark.parametrize("freq,rate", [(20.0, 25.0), (20.0, 30.0), (20.0, 39.999), (0.0, 100.0), (-1.0, 100.0), (20.0, 0.0), (20.0, -5.0), (float("nan"), 100.0),
                                       (20.0, float("inf")), (float("inf"), float("inf"))])
def test_the_nyquist_refusal_leaves_the_data_untouched(freq, rate):
    """Coefficients::from_params fails for 2 f0 > fs; the reference ignores the error (essential_matrix.rs:47-48): estimated rates at 25 or 30 fps are never filtered"""
    x = series(50, seed=3)
    keep = x.copy()
    lib = abi.load_library()
    assert lib.gfw_lowpass_gyro(freq, rate, x.ctypes.data, None, len(x)) == abi.FILTER_NOT_APPLIED == 1
    assert same_bits(x, keep)
    got, applied = warp.lowpass_gyro(freq, rate, x)
    assert not applied and same_bits(got, keep)
    assert G.lowpass_gyro(freq, rate, x)[1] is False
    assert lib.gfw_lowpass_gyro(20.0, 40.0, x.ctypes.data, None, len(x)) == 0         # 2 f0 == fs is accepted


def test_bad_arguments():
    lib = abi.load_library()
    assert lib.gfw_lowpass_gyro(20.0, 200.0, None, None, 4) == abi.ERR_INVALID_ARGUMENT
    x = series(4)
    assert lib.gfw_lowpass_gyro(20.0, 200.0, x.ctypes.data, None, -1) == abi.ERR_INVALID_ARGUMENT
    assert b"lowpass" in lib.gfw_last_error()
    assert lib.gfw_lowpass_gyro(20.0, 200.0, None, None, 0) == 0


def test_dc_gain_of_a_step_is_one_after_both_passes():
    n = 20000
    x = np.zeros((n, 3))
    x[:, 0], x[:, 1], x[:, 2] = 1.0, -7.5, 123.0
    got, _ = warp.lowpass_gyro(20.0, 1000.0, x)
    mid = got[n // 2]
    assert np.all(np.abs(mid / np.array([1.0, -7.5, 123.0]) - 1.0) < 1e-12), mid


def test_scipy_lfilter_forward_then_backward_agrees():
    signal = pytest.importorskip("scipy.signal")
    x = series(500, seed=4)
    b0, b1, b2, a1, a2 = G.lowpass_coefficients(20.0, 200.0)
    fwd = signal.lfilter([b0, b1, b2], [1.0, a1, a2], x, axis=0)
    want = signal.lfilter([b0, b1, b2], [1.0, a1, a2], fwd[::-1], axis=0)[::-1]
    got, _ = warp.lowpass_gyro(20.0, 200.0, x)
    assert same_bits(got, want)
