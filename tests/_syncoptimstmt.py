"""TEST INFRASTRUCTURE: numpy statements of OptimSync (src/core/synchronization/optimsync.rs) — where in a clip to sync.

Two forms of ``run`` (:68-225) and one of ``new`` (:30-66):

``literal``  what the reference computes, in f64 with numpy.fft — the measuring stick.  Each axis is cast to f32, multiplied by blackman(N) (N = round(sample_rate)),
    transformed; per window and k < N/2 the bin is |X[k] + X[N-1-k]| * scale (`zip(cm.iter(), cm.iter().rev())`: N-1-k, not N-k; scale = sqrt(1/N)/N*256); the axes
    are merged as (x + y) + z; lf / mf / hf are the sums over bins [b(0), b(2)), [b(2), b(30)), [b(30), b(2000)) with b(f) = round(N / sample_rate * f) clamped to
    0 .. N/2-1 (ends exclusive: bin N/2-1 is never in hf); the rank, the masks, the non-maximum suppression and the picks as ``tail`` states them.

``f32``  what the device, the interpreted kernels and the mirrors compute TO THE BIT.  rustfft's summation order is no contract, so the quantity is restated:
    xw[n] = f32(x[n]) * win[n] (one f32 product); for k = 0 .. N/2, re[k] is the LEFT FOLD over n = 0 .. N-1, from 0.0, of xw[n] * c[(k n) mod N] and im[k] the same
    fold of -(xw[n] * s[(k n) mod N]), every product and sum one f32 operation; c / s are tables of N f32 built on the host in f64 and rounded once — taken FROM
    gfw_optim_tables, as the window is, so that a last-bit difference between numpy's and the C library's cosine cannot enter a bit comparison (tests/test_sync_optim_host.py
    holds the tables to numpy within 1 ulp).  X[N-1-k] of a real input is conj(X[k+1]): sr = re[k] + re[k+1], si = im[k] + (-im[k+1]),
    mag = sqrtf(sr*sr + si*si) * scale with scale evaluated in f32 as the reference writes it.  From there on every operation is the reference's own f32 operation in
    its own order; a band sum is the sequential fold, from 0.0, over the bins in index order.  Point times are f64.

The bound between the two (``band_bound``), per window and band, from the formats alone — u = 2^-24, gamma_j = j u / (1 - j u):
    * a bin's real (or imaginary) part.  With A = sum_n |f32(x[n]) win[n]| of the window and axis, a term xw32[n] * c32[j] carries three roundings (the window
      product, the table entry, the term's product): |term - exact| <= gamma_3 |xw[n]|; the recursive sum of N terms adds at most gamma_N sum |term|
      (Higham, Accuracy and Stability, section 4.2).  Together e_X A with e_X = gamma_(N+3); the f64 transform on the other side is itself off by at most
      N 2^-53 A a part (far above any FFT's bound), which is added to e_X.
    * the pair sum.  Each part adds two such errors and one rounding of a sum of magnitude at most 2 A (1 + e_X): c = (2 e_X + 2 u (1 + e_X)) A a part, sqrt(2) c for
      the complex number.
    * the norm and the scale.  Two squares and their sum are (1 + u)^2 under the root, the root halves that and rounds once, scale in f32 is three roundings off the
      f64 scale (the quotient, its root, the division by N; * 256 is exact) and the product rounds once: a factor within gamma_6, on a magnitude of at most 2 A.
      E_axis = scale A (sqrt(2) (2 e_X + 2 u (1 + e_X)) (1 + gamma_6) + 2 gamma_6).
    * the merge of the axes, two sums: E_bin[k] = E + gamma_2 (merged64[k] + E) with E = E_x + E_y + E_z.
    * the band fold of B bins (B additions, the first to 0.0): sum_k E_bin[k] + gamma_B sum_k (merged64[k] + E_bin[k]).
Nothing measured enters it."""
import ctypes as C
import math

import numpy as np

from gyroflow_amd import abi

HOP = 16
F32 = np.float32
U = 2.0 ** -24


def gamma(j):
    return j * U / (1.0 - j * U)


def tables(n):
    """(win, cos, sin) [n] f32 of gfw_optim_tables (host only: no GPU)"""
    win, c, s = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    rc = abi.load_library().gfw_optim_tables(n, win.ctypes.data, c.ctypes.data, s.ctypes.data)
    assert rc == 0, rc
    return win, c, s


def blackman_numpy(width):
    """blackman() of optimsync.rs:15-27 restated with numpy's f32 cosine (for the 1-ulp comparison of the tables only)"""
    a0, a1, a2 = F32(7938.0) / F32(18608.0), F32(9240.0) / F32(18608.0), F32(1430.0) / F32(18608.0)
    size = F32(width - 1)
    n = np.arange(width).astype(F32)
    pi = F32(math.pi)
    return (a0 - a1 * np.cos(F32(2.0) * pi * n / size, dtype=F32)) + a2 * np.cos(F32(4.0) * pi * n / size, dtype=F32)


def rust_round(v):
    """f64::round: half away from zero"""
    return math.floor(abs(v) + 0.5) * (1.0 if v >= 0 else -1.0)


def as_usize(v):
    return 0 if v != v or v < 1.0 else int(min(v, 2.0 ** 62))


def fft_size(sample_rate):
    return as_usize(rust_round(float(sample_rate)))


def n_windows(n_samples, n):
    return 0 if n_samples < n or n < 1 else (n_samples - n) // HOP + 1


def map_to_bin(n, sample_rate, freq):
    return int(min(max(rust_round(n / sample_rate * freq), 0.0), float(n // 2 - 1)))


def band_bins(n, sample_rate):
    return [map_to_bin(n, sample_rate, f) for f in (0.0, 2.0, 30.0, 2000.0)]


def windows_of(x, n, w):
    """[w][n] view of the windows of a series"""
    return np.lib.stride_tricks.as_strided(x, shape=(w, n), strides=(x.strides[0] * HOP, x.strides[0])) if w else np.zeros((0, n), dtype=x.dtype)


def merged_literal(gyro, sample_rate):
    """-> (merged bins [W][N/2] f64, A [3][W]: sum_n |f32(x[n]) win[n]|)"""
    n = fft_size(sample_rate)
    g = np.asarray(gyro, dtype=np.float64).reshape(3, -1).astype(F32).astype(np.float64)
    w = n_windows(g.shape[1], n)
    win = tables(n)[0].astype(np.float64)
    scale = math.sqrt(1.0 / n) / n * 256.0
    per, absum = [], []
    for a in range(3):
        xw = windows_of(g[a], n, w) * win
        X = np.fft.fft(xw, axis=1)
        per.append(np.abs(X[:, :n // 2] + X[:, ::-1][:, :n // 2]) * scale)
        absum.append(np.sum(np.abs(xw), axis=1))
    return (per[0] + per[1]) + per[2], np.array(absum).reshape(3, w)


def merged_f32(gyro, sample_rate, chunk=64):
    """-> merged bins [W][N/2] f32 of the f32 form"""
    n = fft_size(sample_rate)
    h = n // 2
    g = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1).astype(F32))
    w = n_windows(g.shape[1], n)
    win, c, s = tables(n)
    fs = F32(n)
    scale = np.sqrt(F32(1.0) / fs) / fs * F32(256.0)
    assert scale.dtype == F32
    out = np.zeros((w, h), dtype=F32)
    k = np.arange(h + 1, dtype=np.int64)
    for w0 in range(0, w, chunk):
        w1 = min(w0 + chunk, w)
        xw = np.stack([windows_of(g[a][w0 * HOP:], n, w1 - w0) * win for a in range(3)])          # [3][wc][n], one f32 product each
        re = np.zeros((3, w1 - w0, h + 1), dtype=F32)
        im = np.zeros((3, w1 - w0, h + 1), dtype=F32)
        for i in range(n):
            at = (k * i) % n
            x = xw[:, :, i, None]
            re += x * c[at]
            im += -(x * s[at])
        sr = re[:, :, :-1] + re[:, :, 1:]
        si = im[:, :, :-1] + (-im[:, :, 1:])
        mag = np.sqrt(sr * sr + si * si) * scale
        out[w0:w1] = (mag[0] + mag[1]) + mag[2]
    return out


def band_sums(merged, bins, dtype):
    """lf, mf, hf [W]: sequential folds from 0.0 over the bins in index order"""
    out = []
    for b in range(3):
        acc = np.zeros(merged.shape[0], dtype=dtype)
        for j in range(bins[b], bins[b + 1]):
            acc = acc + merged[:, j]
        out.append(acc)
    return out


def nlfunc(arg, trip):
    return np.where(arg < trip, arg.dtype.type(0.0), arg - trip)


def tail(lf, mf, hf, sample_rate, n, target, trims, dtype):
    """Everything behind the band energies (:134-204), in `dtype` arithmetic -> dict(points, rank, masked, rank_nms, ratio)"""
    T = dtype
    w = len(mf)
    # fold(0.0, f32::max): f32::max ignores a NaN, as fmaxf does, so the fold is total — and among numbers the order does not matter
    mf_max = T(np.fmax.reduce(np.asarray(mf, dtype=T), initial=T(0.0))) if w else T(0.0)
    low_motion = bool(mf_max < T(50.0))
    if low_motion:
        rank = (lf + mf) / (T(1.0) + nlfunc(hf, T(450.0)) * T(0.003))
    else:
        rank = mf / (T(1.0) + nlfunc(hf, T(450.0)) * T(0.003)) / (T(1.0) + nlfunc(lf, T(650.0)) * T(0.003))
    rank = rank.astype(T)
    ratio = HOP / float(sample_rate)
    time = np.arange(w, dtype=np.float64) * ratio
    inside = np.zeros(w, dtype=bool)
    for a, b in np.asarray(trims, dtype=np.float64).reshape(-1, 2):
        inside |= (time >= a) & (time <= b)
    masked = np.where((rank < T(50.0)) | ~inside, T(0.0), rank).astype(T)
    total = w * ratio
    if total > 12.0:
        masked[(time < 2.0) | (time >= (total - 2.0))] = T(0.0)
    r = as_usize((float(sample_rate) / 16.0 / 2.0) * 8.0)
    rank_nms = masked.copy()
    for j in range(w - 1):                                                           # the last element is never cleared
        lo, hi = max(j - r + 1, 0), min(j + r, w - 1)
        if hi >= lo and np.any(masked[j] < masked[lo:hi + 1]):
            rank_nms[j] = T(0.0)
    points = []
    seg = (w + target - 1) // target
    seg_pick = np.full(target, -1, dtype=np.int64)                                   # the window a segment's point stands for, -1 without one
    for i in range(target):
        start = i * seg
        end = min(start + seg, w)
        if start > end or end <= start:
            continue
        part = rank_nms[start:end]
        best = 0
        for c in range(1, len(part)):                                                # max_by: the later of equals
            if not (part[best] > part[c]):
                best = c
        if part[best] < T(0.1):
            continue
        seg_pick[i] = start + best
        points.append((float(start + best) * 16.0 + float(n) / 2.0) / float(sample_rate) * 1000.0)
    return dict(points=np.array(points, dtype=np.float64), rank=rank, masked=masked, rank_nms=rank_nms, ratio=ratio, low_motion=low_motion, seg_pick=seg_pick)


def run_literal(gyro, sample_rate, target, trims):
    n = fft_size(sample_rate)
    merged, absum = merged_literal(gyro, sample_rate)
    lf, mf, hf = band_sums(merged, band_bins(n, sample_rate), np.float64)
    out = tail(lf, mf, hf, sample_rate, n, target, trims, np.float64)
    out.update(lf=lf, mf=mf, hf=hf, merged=merged, absum=absum)
    return out


def run_f32(gyro, sample_rate, target, trims):
    n = fft_size(sample_rate)
    merged = merged_f32(gyro, sample_rate)
    lf, mf, hf = band_sums(merged, band_bins(n, sample_rate), F32)
    out = tail(lf, mf, hf, sample_rate, n, target, trims, F32)
    out.update(lf=lf, mf=mf, hf=hf, merged=merged)
    return out


def band_bound(merged64, absum, sample_rate):
    """-> [3][W]: the bound on |f32 - f64| of lf, mf, hf derived in the module docstring"""
    n = fft_size(sample_rate)
    scale = math.sqrt(1.0 / n) / n * 256.0
    e_x = gamma(n + 3) + n * 2.0 ** -53
    g6 = gamma(6)
    e_axis = scale * absum * (math.sqrt(2.0) * (2.0 * e_x + 2.0 * U * (1.0 + e_x)) * (1.0 + g6) + 2.0 * g6)      # [3][W]
    e = e_axis[0] + e_axis[1] + e_axis[2]                                                                           # [W]
    e_bin = e[:, None] + gamma(2) * (merged64 + e[:, None])                                                        # [W][N/2]
    bins = band_bins(n, sample_rate)
    out = []
    for b in range(3):
        lo, hi = bins[b], bins[b + 1]
        cnt = max(hi - lo, 0)
        out.append(np.sum(e_bin[:, lo:hi], axis=1) + gamma(max(cnt, 1)) * np.sum(merged64[:, lo:hi] + e_bin[:, lo:hi], axis=1) if cnt else np.zeros(merged64.shape[0]))
    return np.array(out)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_bits_nan(a, b):
    """same_bits for inputs that may be non-finite: NaNs at the same indices, with any sign or payload (x86 and the GPU may produce different default-NaN bit
    patterns, and which operand's payload an operation forwards is no contract); every other element equal as a uint32 / uint64 view"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        return False
    na, nb = np.isnan(a), np.isnan(b)
    view = np.uint32 if a.dtype == np.dtype(np.float32) else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(view)[~na], b.view(view)[~nb]))


# ---- OptimSync::new ----
def resample(timestamps_ms, xyz, has=None):
    """-> (gyro [3][S] f64, sample_rate): f64, the reference's operation order"""
    ts = np.asarray(timestamps_ms, dtype=np.float64).reshape(-1)
    v = np.asarray(xyz, dtype=np.float64).reshape(-1, 3).copy()
    n = len(ts)
    present = np.ones(n, dtype=bool) if has is None else (np.asarray(has).reshape(-1) != 0)
    v[~present] = 0.0                                                                # unwrap_or_default
    duration = ts[-1] - ts[0]
    with np.errstate(all="ignore"):
        sr = np.float64(np.count_nonzero(present)) / duration * 1000.0
        count = as_usize(float(duration * sr / 1000.0))
        t = np.arange(count, dtype=np.float64) * 1000.0 / sr
    i_r = np.minimum(np.searchsorted(ts, t, side="left"), n - 1)
    i_l = np.maximum(i_r, 1) - 1
    out = np.zeros((3, count))
    for a in range(3):
        with np.errstate(all="ignore"):
            two = (v[i_l, a] * (ts[i_r] - t) + v[i_r, a] * (t - ts[i_l])) / (ts[i_r] - ts[i_l])
        out[a] = np.where(i_l == i_r, v[i_l, a], two)
    return out, float(sr)


def lib_resample(timestamps_ms, xyz, has=None):
    """gfw_optim_resample -> (gyro [3][S] f64, sample_rate)"""
    ts = np.ascontiguousarray(np.asarray(timestamps_ms, dtype=np.float64).reshape(-1))
    v = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    h = None if has is None else np.ascontiguousarray((np.asarray(has).reshape(-1) != 0).astype(np.uint8))
    lib = abi.load_library()
    n_out, sr = C.c_int64(-1), C.c_double(-1.0)
    args = (ts.ctypes.data, v.ctypes.data, h.ctypes.data if h is not None else None, len(ts))
    rc = lib.gfw_optim_resample(*args, None, 0, C.addressof(n_out), C.addressof(sr))
    assert rc == 0, (rc, lib.gfw_last_error())
    out = np.full((3, n_out.value), -7.0)
    rc = lib.gfw_optim_resample(*args, out.ctypes.data if out.size else None, n_out.value, C.addressof(n_out), C.addressof(sr))
    assert rc == 0, (rc, lib.gfw_last_error())
    return out, sr.value


# ---- planted clips ----
BURSTS_S = (7.0, 19.0, 33.0, 48.0)
PLANTED = ((200.0, 60.0), (97.3, 45.0), (400.0, 30.0))                                # (rate Hz, duration s)


def planted_clip(rate, duration_s, seed=0):
    """gyro [3][S]: N(0, 0.3) noise and Gaussian-envelope bursts (sigma 0.8 s) of 40-60 deg/s at 5-11 Hz centred at BURSTS_S -> (gyro, the centres inside the clip).

    A burst is ONE oscillation seen by the three axes a third of a period apart.  The reason is the reference's bin pairing: X[k] + X[N-1-k] = X[k] + conj(X[k+1]) of
    a sinusoid is a e^(i phi) + b e^(-i phi) with phi its phase at the window's first sample, so one axis's magnitude swings between |a| - |b| and |a| + |b| as the
    window hops, by far more than the envelope (sigma 0.8 s) falls within two hops — the maximum of a single axis lands anywhere on the burst's flat top.  Three axes
    120 degrees apart leave the third harmonic of that swing only.  What remains still depends on the draw: of the seeds 0 .. 15 of this generator, 12 put every
    burst within two hops and 4 within 2.5 (tried once with the literal form, before any kernel existed); the tests use seed 0."""
    rs = np.random.RandomState(1000 + seed)
    s = int(rate * duration_s)
    t = np.arange(s) / rate
    g = rs.normal(0.0, 0.3, (3, s))
    for c in BURSTS_S:
        amp, freq, phase = rs.uniform(40.0, 60.0), rs.uniform(5.0, 11.0), rs.uniform(0.0, 2.0 * math.pi)
        env = np.exp(-0.5 * ((t - c) / 0.8) ** 2)
        for a in range(3):
            g[a] += amp * env * np.sin(2.0 * math.pi * freq * t + phase + a * 2.0 * math.pi / 3.0)
    return g, [c for c in BURSTS_S if c < duration_s]
