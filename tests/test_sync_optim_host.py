"""The host-only helpers of the sync-point choice (gyroflow_amd/csrc/gfw_sync_optim_host.h behind gfw_optim_tables / gfw_optim_resample): the Blackman window and the
twiddle tables against numpy within 1 f32 ulp — the statements take their tables FROM the library, so this is where the tables themselves are held — and
OptimSync::new's resampling against a numpy restatement to the bit (f64, the reference's operation order).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi
import _syncoptimstmt as S


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("n", [16, 97, 200, 1000, 8192])
def test_tables_equal_numpy_within_one_ulp(n):
    win, c, s = S.tables(n)
    j = np.arange(n, dtype=np.float64)
    assert np.array_equal(c, np.cos(2.0 * np.pi * j / n).astype(np.float32)) or ulps(c, np.cos(2.0 * np.pi * j / n).astype(np.float32)).max() <= 1.0
    assert ulps(s, np.sin(2.0 * np.pi * j / n).astype(np.float32)).max() <= 1.0
    assert c[0] == 1.0 and s[0] == 0.0
    # the window: every operation is one f32 operation of optimsync.rs:15-27; numpy's f32 cosine may differ from the C library's in the last bit, which the two
    # products and sums carry to at most one ulp of the largest term (a0 + a1 + a2 = 1)
    ref = S.blackman_numpy(n)
    assert np.max(np.abs(win.astype(np.float64) - ref.astype(np.float64))) <= 2.0 ** -23
    exact = 7938.0 / 18608.0 - 9240.0 / 18608.0 * np.cos(2.0 * np.pi * j / (n - 1)) + 1430.0 / 18608.0 * np.cos(4.0 * np.pi * j / (n - 1))
    assert np.max(np.abs(win - exact)) < 1e-5 and 0.95 < win.max() <= 1.0 and abs(win[0] - 128.0 / 18608.0) < 1e-6


def test_tables_reject_sizes_outside_their_range_and_take_null_arrays():
    lib = abi.load_library()
    buf = np.full(8, -7.0, dtype=np.float32)
    for n in (15, 8193, 0, -3):
        assert lib.gfw_optim_tables(n, buf.ctypes.data, None, None) == abi.ERR_INVALID_ARGUMENT and b"fft_size" in lib.gfw_last_error()
    assert np.all(buf == -7.0)
    win = np.zeros(16, dtype=np.float32)
    assert lib.gfw_optim_tables(16, None, None, None) == 0 and lib.gfw_optim_tables(16, win.ctypes.data, None, None) == 0
    assert S.same_bits(win, S.tables(16)[0])


def series(n, rate, seed, jitter=0.2):
    rs = np.random.RandomState(seed)
    ts = 1000.0 / rate * (np.arange(n) + rs.uniform(-jitter, jitter, n)) + 3.25
    return np.sort(ts), rs.normal(0.0, 20.0, (n, 3))


def check(ts, xyz, has=None):
    got, sr = S.lib_resample(ts, xyz, has)
    want, wsr = S.resample(ts, xyz, has)
    assert (sr == wsr or (sr != sr and wsr != wsr)) and S.same_bits(got, want), (sr, wsr, got.shape, want.shape)
    return got, sr


def test_resample_equals_the_restatement_to_the_bit():
    ts, xyz = series(500, 200.0, 1)
    got, sr = check(ts, xyz)
    assert abs(sr - 200.0) < 1.0 and got.shape == (3, 500)
    assert S.same_bits(got[:, 0], xyz[0])                                                # t = 0 lies before the first sample: i_l == i_r == 0


def test_resample_with_missing_gyro_values():
    ts, xyz = series(400, 100.0, 2)
    has = np.ones(400, dtype=np.uint8)
    has[::7] = 0
    has[50:60] = 0
    got, sr = check(ts, xyz, has)
    assert sr < 90.0 and got.shape[1] == int((ts[-1] - ts[0]) * sr / 1000.0)             # the rate counts the samples that have a value
    all_in, sr_all = check(ts, xyz)
    assert sr_all > sr and not S.same_bits(got[:, :50], all_in[:, :50])                  # a None side counts as zeros


def test_resample_of_a_single_sample_and_of_equal_timestamps():
    lib = abi.load_library()
    got, sr = check(np.array([5.0]), np.array([[1.0, 2.0, 3.0]]))                        # duration 0: the rate is 1 / 0, no samples
    assert got.shape == (3, 0) and sr == float("inf")
    got, sr = check(np.array([5.0, 5.0]), np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]))
    assert got.shape == (3, 0) and sr == float("inf")
    got, sr = check(np.array([5.0]), np.array([[1.0, 2.0, 3.0]]), has=[0])               # 0 / 0
    assert got.shape == (3, 0) and sr != sr
    n_out, rate = C.c_int64(-7), C.c_double(-7.0)
    assert lib.gfw_optim_resample(None, None, None, 0, None, 0, C.addressof(n_out), C.addressof(rate)) == abi.ERR_INVALID_ARGUMENT
    assert n_out.value == -7 and rate.value == -7.0 and b"OptimSync::new" in lib.gfw_last_error()
    ts, xyz = series(50, 100.0, 3)
    small = np.full((3, 10), -7.0)
    assert lib.gfw_optim_resample(ts.ctypes.data, xyz.ctypes.data, None, 50, small.ctypes.data, 10, C.addressof(n_out), C.addressof(rate)) == abi.ERR_INVALID_ARGUMENT
    assert np.all(small == -7.0) and n_out.value == -7 and b"out_stride" in lib.gfw_last_error()


def test_resample_feeds_the_statement():
    ts, xyz = series(1200, 100.0, 4, jitter=0.0)
    got, sr = check(ts, xyz)
    assert S.fft_size(sr) == 100 and S.n_windows(got.shape[1], 100) > 60
