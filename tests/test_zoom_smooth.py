"""gfw_zoom_smooth (zooming/mod.rs:55-68 + zoom_dynamic.rs on the host; no context, no GPU) against the Python statement: bit-identical."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, warp
import _zoomstmt as Z


def series(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return 1.0 + 0.2 * np.sin(t * 0.11) + 0.1 * rng.random(n) - 0.3 * (rng.random(n) < 0.03)


@pytest.mark.parametrize("n", [1, 2, 1000])
@pytest.mark.parametrize("fps", [24.0, 30.0, 59.94])
@pytest.mark.parametrize("method", [0, 1])
def test_bit_identical_to_the_statement(n, fps, method):
    v = series(n, 7 + n)
    for window in (0.0, -1.0, 0.5, 2.0, 8.0):
        for ranges in ((), [(0.1, 0.4), (0.7, 0.95)]):
            ref_f, ref_m = Z.zoom_smooth(v, window, fps, method, ranges)
            got_f, got_m = warp.zoom_smooth(v, window, fps, method, ranges)
            assert got_f.tolist() == ref_f, (n, fps, method, window, ranges)
            assert got_m.tolist() == ref_m, (n, fps, method, window, ranges)


def test_bad_arguments_are_rejected():
    lib = abi.load_library()
    v, out = np.ones(4), np.zeros(4)
    f = lib.gfw_zoom_smooth
    assert f(None, 4, 1.0, 30.0, 0, None, 0, out.ctypes.data, None) == abi.ERR_INVALID_ARGUMENT
    assert b"zoom_smooth" in lib.gfw_last_error()
    assert f(v.ctypes.data, 4, 1.0, 30.0, 0, None, 0, None, None) == abi.ERR_INVALID_ARGUMENT
    assert f(v.ctypes.data, -1, 1.0, 30.0, 0, None, 0, out.ctypes.data, None) == abi.ERR_INVALID_ARGUMENT
    assert f(v.ctypes.data, 4, 1.0, 30.0, 0, None, 2, out.ctypes.data, None) == abi.ERR_INVALID_ARGUMENT
    assert f(v.ctypes.data, 4, 1.0, 0.0, 0, None, 0, out.ctypes.data, None) == abi.ERR_INVALID_ARGUMENT
    assert f(v.ctypes.data, 4, float("nan"), 30.0, 0, None, 0, out.ctypes.data, None) == abi.ERR_INVALID_ARGUMENT
    assert np.all(out == 0.0)
    assert f(None, 0, 1.0, 30.0, 0, None, 0, None, None) == 0                      # n = 0: nothing to do
    assert f(v.ctypes.data, 4, 1.0, 30.0, 7, None, 0, out.ctypes.data, None) == 0   # an unknown method is the Gaussian filter (ZoomMethod::from)
    assert out.tolist() == Z.zoom_smooth(v, 1.0, 30.0, 0)[0]
