"""TEST INFRASTRUCTURE: a numpy statement of the gyro-match offset search (src/core/synchronization/find_offset/essential_matrix.rs:13-131), of the low-pass it
runs first (filtering.rs:46-74 over the biquad crate's documented Butterworth low-pass) and of the fast initial offset of rs-sync (rs_sync.rs:26-45), written from
those lines; and the planted clips that hold it to what it is for (tests/test_sync_gyro_statement.py).  Every sum is the reference's own sequential f64 fold:
the costs of many candidates are evaluated side by side (numpy arrays over the candidates), never reassociated.  Not a product path."""
import math

import numpy as np

F64_MAX = float(np.finfo(np.float64).max)
FINE = 200
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the low-pass ----------------------------------------------------------------------------------------------------------------------------------------------------
def lowpass_coefficients(freq, sample_rate):
    """biquad 0.6.0 Coefficients::<f64>::from_params(Type::LowPass, fs, f0, Q_BUTTERWORTH_F64), restated from the crate's documented form -> (b0, b1, b2, a1, a2)
    divided by a0, or None where it returns Err (2 f0 > fs; a negative Q does not arise)"""
    if not (math.isfinite(freq) and math.isfinite(sample_rate)) or not freq > 0.0 or not sample_rate > 0.0 or 2.0 * freq > sample_rate:
        return None
    omega = 2.0 * math.pi * freq / sample_rate
    omega_s, omega_c = math.sin(omega), math.cos(omega)
    alpha = omega_s / (2.0 * 0.7071067811865476)
    b0, b1, b2 = (1.0 - omega_c) * 0.5, 1.0 - omega_c, (1.0 - omega_c) * 0.5
    a0, a1, a2 = 1.0 + alpha, -2.0 * omega_c, 1.0 - alpha
    return b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0


def lowpass_gyro(freq, sample_rate, xyz, has=None):
    """Lowpass::filter_gyro_forward_backward of the gyro triples: -> (float64 [n][3], applied).  DirectForm2Transposed::run, a filter per axis and direction;
    entries without a gyro are skipped and do not advance the state."""
    v = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    co = lowpass_coefficients(freq, sample_rate)
    if co is None:
        return v, False
    b0, b1, b2, a1, a2 = co
    n = len(v)
    for order in (range(n), range(n - 1, -1, -1)):
        for a in range(3):
            s1 = s2 = 0.0
            for i in order:
                if has is not None and not has[i]:
                    continue
                x = float(v[i, a])
                out = s1 + b0 * x
                s1 = s2 + b1 * x - a1 * out
                s2 = b2 * x - a2 * out
                v[i, a] = out
    return v, True


# ---- the cost and the search -----------------------------------------------------------------------------------------------------------------------------------------
def key(v):
    """`v as usize`: truncating, saturating, NaN -> 0"""
    if not v >= 1.0:
        return 0
    return 0xFFFFFFFFFFFFFFFF if v >= 18446744073709551616.0 else int(v)


def keys_of(v):
    """key() over an array -> uint64"""
    v = np.asarray(v, dtype=np.float64)
    small = ~(v >= 1.0)
    big = v >= 18446744073709551616.0
    out = np.where(small | big, 0.0, v).astype(np.uint64)
    out[big] = U64_MAX
    return out


class Tree:
    """BTreeMap<usize, TimeIMU> of :50: keys ascending; a later sample with the same key replaces an earlier one"""

    def __init__(self, gyro, gyro_has=None):
        g = np.asarray(gyro, dtype=np.float64).reshape(-1, 4)
        has = np.ones(len(g), dtype=bool) if gyro_has is None else np.asarray(gyro_has).reshape(-1) != 0
        m = {}
        for i in range(len(g)):
            m[key(float(g[i, 0]) * 1000.0)] = i
        ks = sorted(m)
        at = [m[k] for k in ks]
        self.keys = np.array(ks, dtype=np.uint64)
        self.values = g[at, 1:] if at else np.zeros((0, 3))
        self.has = has[at] if at else np.zeros(0, dtype=bool)


def cost_scalar(offs, est, est_has, tree):
    """calculate_cost (:109-131) of one candidate, line by line"""
    est = np.asarray(est, dtype=np.float64).reshape(-1, 4)
    total, matches = 0.0, 0
    for j in range(len(est)):
        q = key((float(est[j, 0]) - offs) * 1000.0)
        at = int(np.searchsorted(tree.keys, np.uint64(q), side="left"))
        if at >= len(tree.keys):
            continue
        if tree.has[at] and (est_has is None or est_has[j]):
            g, o = tree.values[at], est[j, 1:]
            matches += 1
            total += (float(g[0] - o[0]) * float(g[0] - o[0])) * 70.0                       # :117-119: three separate additions, `powi(2)` = x * x
            total += (float(g[1] - o[1]) * float(g[1] - o[1])) * 70.0
            total += (float(g[2] - o[2]) * float(g[2] - o[2])) * 100.0
    if len(est) and matches > len(est) // 2:
        return total / float(matches)
    return F64_MAX


def costs(cands, est, est_has, tree):
    """calculate_cost of every candidate: the candidates side by side, the samples one after another — each candidate's sum is the sequential fold of cost_scalar"""
    cands = np.asarray(cands, dtype=np.float64).reshape(-1)
    est = np.asarray(est, dtype=np.float64).reshape(-1, 4)
    total = np.zeros(len(cands))
    matches = np.zeros(len(cands), dtype=np.int64)
    nk = len(tree.keys)
    with np.errstate(all="ignore"):
        for j in range(len(est)):
            if nk == 0 or not (est_has is None or est_has[j]):
                continue
            at = np.searchsorted(tree.keys, keys_of((est[j, 0] - cands) * 1000.0), side="left")
            hit = at < nk
            at = np.minimum(at, nk - 1)
            hit &= tree.has[at]
            g = tree.values[at]
            matches += hit
            for a, w in ((0, 70.0), (1, 70.0), (2, 100.0)):
                d = g[:, a] - est[j, 1 + a]
                total = np.where(hit, total + (d * d) * w, total)
        out = total / matches.astype(np.float64)
    return np.where((len(est) > 0) & (matches > len(est) // 2), out, F64_MAX)


def find_min(values):
    """`reduce_with(find_min)`, `if a.1 < b.1 { a } else { b }` under an order-preserving reduce: the index of the LAST minimal value"""
    best = 0
    for i in range(1, len(values)):
        if not values[best] < values[i]:
            best = i
    return best


def coarse_candidates(initial_offset, search_size):
    steps = key(search_size) * 2                                              # `search_size as usize * 2` (:55)
    return (initial_offset - search_size) + np.arange(steps, dtype=np.float64)               # :59


def fine_candidates(lowest):
    step = 2.0 / float(FINE)                                                  # :65-67
    return lowest + (-2.0 + (np.arange(FINE, dtype=np.float64) * step))      # :71


def search(est, est_has, gyro, gyro_has, initial_offset, search_size):
    """:50-75 of one range -> dict(found, n_coarse, coarse_pick, coarse_value, coarse_cost, fine_pick, value, cost, coarse_costs, fine, fine_costs)"""
    tree = Tree(gyro, gyro_has)
    cc = coarse_candidates(initial_offset, search_size)
    out = {"found": 0, "n_coarse": len(cc), "coarse_costs": np.zeros(0), "fine": np.zeros(FINE), "fine_costs": np.zeros(FINE), "coarse_value": 0.0, "coarse_cost": 0.0,
           "value": 0.0, "cost": 0.0}
    if not len(cc):
        return out
    c = costs(cc, est, est_has, tree)
    ci = find_min(c)
    fine = fine_candidates(cc[ci])
    f = costs(fine, est, est_has, tree)
    fi = find_min(f)
    out.update(found=1, coarse_costs=c, coarse_pick=ci, coarse_value=float(cc[ci]), coarse_cost=float(c[ci]), fine=fine, fine_costs=f, fine_pick=fi,
               value=float(fine[fi]), cost=float(f[fi]))
    return out


# ---- find_offsets (:13-91) and the fast initial offset ---------------------------------------------------------------------------------------------------------------
def max_angle(items):
    m = 0.0
    for _, g in items:
        if g is not None:
            for v in g:
                if abs(v) > m:
                    m = abs(v)
    return m


def _filtered(freq, rate, items):
    has = np.array([g is not None for _, g in items], dtype=bool)
    xyz = np.array([g if g is not None else (0.0, 0.0, 0.0) for _, g in items], dtype=np.float64).reshape(-1, 3)
    out, applied = lowpass_gyro(freq, rate, xyz, has)
    rows = np.zeros((len(items), 4))
    rows[:, 0] = [t for t, _ in items]
    rows[:, 1:] = out
    return rows, has, applied


def range_inputs(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, initial_offset, search_size):
    """:13-48 -> [dict(index, est, est_has, gyro, gyro_has, est_filtered, gyro_filtered)] of the ranges that reach the search"""
    out = []
    if not estimated_gyro or not duration_ms > 0.0 or not len(raw_imu):
        return out
    ks = sorted(estimated_gyro)
    for i, (from_ts, to_ts) in enumerate(ranges):
        if to_ts <= from_ts:
            continue
        of_item = [estimated_gyro[k] for k in ks if from_ts <= k < to_ts]
        if not of_item:
            continue
        lo, hi = of_item[0][0] - search_size, of_item[-1][0] + search_size
        gyro_item = [x for x in raw_imu if lo <= x[0] + initial_offset <= hi]
        if max_angle(of_item) < 3.0:
            continue
        sample_rate = float(len(raw_imu)) / (duration_ms / 1000.0)
        est, est_has, ef = _filtered(20.0, scaled_fps, of_item)
        gyro, gyro_has, gf = _filtered(20.0, sample_rate, gyro_item)
        out.append(dict(index=i, est=est, est_has=est_has, gyro=gyro, gyro_has=gyro_has, est_filtered=ef, gyro_filtered=gf))
    return out


def find_offsets(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, initial_offset, search_size, rejected=None):
    """-> [(middle timestamp, offset, cost)]; `rejected`: a list that receives the (range index, offset) the 90 % rule turns away"""
    out = []
    for r in range_inputs(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, initial_offset, search_size):
        s = search(r["est"], r["est_has"], r["gyro"], r["gyro_has"], initial_offset, search_size)
        if not s["found"]:
            continue
        from_ts, to_ts = ranges[r["index"]]
        middle = (float(from_ts) + float(to_ts - from_ts) / 2.0) / 1000.0
        if abs(s["value"] - initial_offset) < search_size * 0.9:
            out.append((middle, s["value"], s["cost"]))
        elif rejected is not None:
            rejected.append((r["index"], s["value"]))
    return out


def median(values):
    v = sorted(values)
    n = len(v)
    return (v[n // 2 - 1] + v[n // 2]) / 2.0 if n % 2 == 0 else v[n // 2]


def initial_offset_fast(offsets, initial_offset, search_size):
    """rs_sync.rs:38-44 over the offsets found"""
    if offsets:
        return median([o for _, o, _ in offsets]), 3000.0
    return initial_offset, search_size


# ---- planted clips ---------------------------------------------------------------------------------------------------------------------------------------------------
def planted_signal(seed, scale=1.0):
    """a smooth gyro: per axis a sum of four sinusoids, 0.3 - 4 Hz, 5 - 25 deg/s each -> f(t_ms) -> [n][3]"""
    rng = np.random.RandomState(seed)
    freq = rng.uniform(0.3, 4.0, size=(3, 4))
    amp = rng.uniform(5.0, 25.0, size=(3, 4)) * scale
    phase = rng.uniform(0.0, 2.0 * math.pi, size=(3, 4))

    def f(t_ms):
        t = np.asarray(t_ms, dtype=np.float64).reshape(-1, 1, 1) / 1000.0
        return np.sum(amp * np.sin(2.0 * math.pi * freq * t + phase), axis=2)
    return f


class Clip:
    """`duration_s` of gyro at `rate` Hz; estimated rates at `fps` that are that gyro delayed by `offset_ms`: est(ts) = gyro(ts - offset_ms)"""

    def __init__(self, fps, rate, offset_ms, seed, duration_s=20.0, scale=1.0, span=((9.0, 10.5),)):
        self.fps, self.rate, self.offset_ms, self.duration_ms = float(fps), float(rate), float(offset_ms), duration_s * 1000.0
        f = planted_signal(seed, scale)
        gt = np.arange(int(duration_s * rate), dtype=np.float64) * 1000.0 / rate
        gv = f(gt)
        self.raw_imu = [(float(t), (float(v[0]), float(v[1]), float(v[2]))) for t, v in zip(gt, gv)]
        et = np.arange(int(duration_s * fps), dtype=np.float64) * 1000.0 / fps
        ev = f(et - offset_ms)
        self.estimated_gyro = {int(round(t * 1000.0)): (float(t), (float(v[0]), float(v[1]), float(v[2]))) for t, v in zip(et, ev)}
        self.ranges = [(int(a * 1e6), int(b * 1e6)) for a, b in span]


# (fps, gyro rate, planted offset): every fps of the issue, rates 200 Hz - 2 kHz, offsets of both signs from 0 to +-2000 ms
PLANTED = [(25.0, 200.0, 0.0), (30.0, 500.0, 7.3), (50.0, 800.0, -133.37), (59.94, 1000.0, 412.6), (60.0, 1600.0, -871.25), (120.0, 2000.0, 1999.5),
           (30.0, 2000.0, -2000.0), (60.0, 200.0, 1500.2), (120.0, 500.0, -1234.56), (25.0, 1000.0, 0.45), (59.94, 400.0, -0.77), (50.0, 2000.0, 1000.0)]


def planted(i):
    fps, rate, offs = PLANTED[i]
    return Clip(fps, rate, offs, seed=100 + i)


# ---- small ranges for the kernel tiers --------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def make_range(n_est, n_gyro, seed=0, fps=59.94, rate=1000.0, start_ms=2000.0, offset_ms=12.3, gyro_from_ms=None):
    """(est [n][4], est_has, gyro [m][4], gyro_has): the estimated rates are the gyro's signal delayed by offset_ms; fps 59.94: timestamps whose * 1000 is no integer"""
    f = planted_signal(seed)
    et = start_ms + np.arange(n_est, dtype=np.float64) * 1000.0 / fps
    est = np.concatenate([et.reshape(-1, 1), f(et - offset_ms)], axis=1) if n_est else np.zeros((0, 4))
    g0 = start_ms - (n_gyro / 2.0) * 1000.0 / rate + (n_est / 2.0) * 1000.0 / fps if gyro_from_ms is None else gyro_from_ms
    gt = g0 + np.arange(n_gyro, dtype=np.float64) * 1000.0 / rate
    gyro = np.concatenate([gt.reshape(-1, 1), f(gt)], axis=1) if n_gyro else np.zeros((0, 4))
    return est, None, gyro, None


def lead_in(first, data, has, k, fill):
    """the same slices `k` entries further into their arrays: first[0] = k, and in front of it `k` entries (`fill`) that belong to no range"""
    if not k:
        return first, data, has
    pad = np.full((k,) + data.shape[1:], fill, dtype=data.dtype)
    return (first + k).astype(np.int32), np.ascontiguousarray(np.concatenate([pad, data])), (None if has is None else np.ascontiguousarray(np.concatenate([np.ones(k, dtype=np.uint8), has])))
