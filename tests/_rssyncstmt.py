"""Host statement of the rs-sync offset search (offset method 2, find_offset/rs_sync.rs) — the checker of gfw_sync_rs_costs / gfw_sync_rs_search.  Test
infrastructure: independent of the device code; not part of the product package.

The reference's adapter (rs_sync.rs) hands per-point unit bearings and per-point timestamps to the `rs-sync` crate, which is NOT in the reference tree: its solver
is not reproduced.  What is mirrored is the adapter — what goes in (:115-146), what comes out and the acceptance rule (:164-184).  The solver is stated here,
operation by operation, and pinned only by itself and by what it is for: tests/test_rs_sync_statement.py holds it to finding planted delays before anything is
compared with it.

  prepare    both frames' points through the lens inverse as tests/_posessstmt.prepare takes it ((-1e6, -1e6) where the inverse is None); the f32 (x, y) give the
             f64 unit bearing of (x, y, 1); the point's time is pair_ts / 1e6 + readout_s * (y_raw / flow_height), y_raw the flow pixel's own y (:132-133)
  lookup     the track (seconds ascending, (w, x, y, z) f64) at t: t clamped to the track's ends, the segment i with T[i] <= t (i <= n - 2), normalised linear
             interpolation with the shorter-arc flip, one sqrt.  World bearing: R(q) diag(1, -1, -1) p
  pair cost  m_i = ra_i x rb_i at t_i + d; direction hypotheses: 0 = the eigenvector of the smallest eigenvalue of sum m m^T (cyclic Jacobi, a fixed number of
             sweeps, the first of equal eigenvalues), h = 1 .. H: m_i x m_j normalised, i = 7h mod n, j = (13h + 5) mod n, skipped where its squared length is
             not > 0; score sum rho(k m_i.t), rho(x) = x^2 / (1 + x^2), the first minimal hypothesis wins; `refits` refits with w_i = 1 / (1 + x_i^2)^2; the
             cost is the score at the last t.  0 points cost 0.0; 1 point has hypothesis 0 only
  sums       every sum over a pair's points: lane l of 64 folds the points l, l + 64, .. from 0.0, then the butterfly v = v + v[l ^ off], off = 32 .. 1
  range      the pairs' costs added in pair order from 0.0
  search     round 0: 2h + 1 candidates initial + (i - h) step, h = floor(radius / step); each later round 17 candidates pick + (i - 8) (step / 8), the step
             divided by 8 again each round; the FIRST minimal candidate wins; behind the last round the vertex of the parabola through the pick and its two
             neighbours where both exist and the second difference is positive

Arithmetic: float64, one rounding per written operator (+ - * / sqrt only), batched over candidates and points (elementwise operations round like scalar ones).
The statement asserts its indices, positive square-root arguments and finite results while it runs.  With `nonfinite=True` (tests/_rstablecase.py) the last two are
off and a NaN goes through as the device's arithmetic takes it: a zero quaternion gives 0 / 0 = NaN, a NaN cost is a NaN range sum.

NaN rule of the pick: a candidate whose range sum is NaN is never picked while another candidate of that round has a sum that is not NaN — the pick is the first
minimum, in candidate order, among the sums that are not NaN; where every sum of a round is NaN the pick is candidate 0 and its cost NaN (`found` stays 1).  The
parabola is skipped where `den > 0.0` is false, so a NaN neighbour means no refinement."""
import numpy as np

import _posessstmt as ES

LANES = 64
LATER = 17                                                                            # candidates of every round behind the first


class Cfg:
    """The solver's settings (gfw_sync_rs_cfg's)"""

    def __init__(self, step_s=3.0 / 1000.0, rounds=4, refine=1, loss_scale=1000.0, hypotheses=16, refits=3, sweeps=5, readout_ms=0.0):
        self.step_s, self.rounds, self.refine, self.loss_scale = float(step_s), int(rounds), int(refine), float(loss_scale)
        self.hypotheses, self.refits, self.sweeps, self.readout_ms = int(hypotheses), int(refits), int(sweeps), float(readout_ms)


def track_seconds(ts_us):
    return np.asarray(ts_us, dtype=np.int64).astype(np.float64) / 1000000.0


def prepare(cam, cfg, pair_ts_us, points_a, points_b):
    """-> (bearings a [n][3], times a [n], bearings b, times b) f64 of one pair"""
    a, b = np.asarray(points_a, dtype=np.float32).reshape(-1, 2), np.asarray(points_b, dtype=np.float32).reshape(-1, 2)
    und = ES.prepare(cam, a, b).astype(np.float64)
    readout_s = cfg.readout_ms / 1000.0
    height = float(cam.flow[1])
    out = []
    for k, pts in enumerate((a, b)):
        t = (float(pair_ts_us[k]) / 1000000.0) + (readout_s * (pts[:, 1].astype(np.float64) / height))
        out += [ES.bearing(und[:, 2 * k], und[:, 2 * k + 1]), t]
    return tuple(out)


def quat_at(T, Q, t, conj=False, nonfinite=False):
    """the track at the times t [..] -> (w, x, y, z) arrays"""
    if nonfinite:
        with np.errstate(all="ignore"):
            return _quat_at(T, Q, t, conj, True)
    return _quat_at(T, Q, t, conj, False)


def _quat_at(T, Q, t, conj, nonfinite):
    n = len(T)
    assert n >= 2
    tc = np.where(t < T[0], T[0], np.where(t > T[n - 1], T[n - 1], t))
    i = np.clip(np.searchsorted(T, tc, side="right") - 1, 0, n - 2)
    assert (i >= 0).all() and (i <= n - 2).all()
    f = (tc - T[i]) / (T[i + 1] - T[i])
    a, b = [Q[i, k] for k in range(4)], [Q[i + 1, k] for k in range(4)]
    dot = (((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])) + (a[3] * b[3])
    b = [np.where(dot < 0.0, -x, x) for x in b]
    q = [x + ((y - x) * f) for x, y in zip(a, b)]
    s = (((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])) + (q[3] * q[3])
    assert nonfinite or (s > 0.0).all()
    nrm = np.sqrt(s)
    q = [x / nrm for x in q]
    if conj:
        q = [q[0], -q[1], -q[2], -q[3]]
    return q


def to_world(q, p):
    """R(q) diag(1, -1, -1) p; p [n][3] broadcast against q [..][n]"""
    w, x, y, z = q
    p0, p1, p2 = p[:, 0], -p[:, 1], -p[:, 2]
    r00, r01, r02 = 1.0 - (2.0 * ((y * y) + (z * z))), 2.0 * ((x * y) - (w * z)), 2.0 * ((x * z) + (w * y))
    r10, r11, r12 = 2.0 * ((x * y) + (w * z)), 1.0 - (2.0 * ((x * x) + (z * z))), 2.0 * ((y * z) - (w * x))
    r20, r21, r22 = 2.0 * ((x * z) - (w * y)), 2.0 * ((y * z) + (w * x)), 1.0 - (2.0 * ((x * x) + (y * y)))
    return (((r00 * p0) + (r01 * p1)) + (r02 * p2), ((r10 * p0) + (r11 * p1)) + (r12 * p2), ((r20 * p0) + (r21 * p1)) + (r22 * p2))


def wave_sum(v):
    """v [C][n] -> [C]: lane-strided partial sums from 0.0, then the butterfly"""
    C, n = v.shape
    acc = np.zeros((C, LANES))
    for base in range(0, n, LANES):
        k = min(LANES, n - base)
        acc[:, :k] = acc[:, :k] + v[:, base:base + k]
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    return acc[:, 0].copy()


def smallest(M6, sweeps):
    """M6: the six sums (00, 01, 02, 11, 12, 22), [C] each -> t [C][3]: the eigenvector of the smallest eigenvalue, the first of equal ones"""
    C = len(M6[0])
    A = np.zeros((C, 3, 3))
    for (i, j), v in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), M6):
        A[:, i, j] = A[:, j, i] = v
    d, V = ES.jacobi(A, sweeps)
    low, e = d[:, 0].copy(), V[:, :, 0].copy()
    for i in (1, 2):
        c = d[:, i] < low
        low, e = np.where(c, d[:, i], low), np.where(c[:, None], V[:, :, i], e)
    return e


def moments(m, w=None):
    prods = [m[i] * m[j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return [wave_sum(p if w is None else w * p) for p in prods]


def residual2(cfg, m, t):
    """x_i^2 of every point under the directions t [C][3] -> [C][n]"""
    x = cfg.loss_scale * (((m[0] * t[:, 0, None]) + (m[1] * t[:, 1, None])) + (m[2] * t[:, 2, None]))
    return x * x


def score(cfg, m, t):
    x2 = residual2(cfg, m, t)
    return wave_sum(x2 / (1.0 + x2))


def pair_costs(cfg, T, Q, prepared, delays, conj=False, directions=False, nonfinite=False):
    """the cost of one pair at the delays [C] (seconds) -> [C] (with `directions` also the final t [C][3])"""
    if nonfinite:
        with np.errstate(all="ignore"):
            return _pair_costs(cfg, T, Q, prepared, delays, conj, directions, True)
    return _pair_costs(cfg, T, Q, prepared, delays, conj, directions, False)


def _pair_costs(cfg, T, Q, prepared, delays, conj, directions, nonfinite):
    ba, ta, bb, tb = prepared
    d = np.asarray(delays, dtype=np.float64).reshape(-1)
    C, n = len(d), len(ta)
    if n == 0:
        return (np.zeros(C), np.zeros((C, 3))) if directions else np.zeros(C)
    ra = to_world(quat_at(T, Q, ta[None, :] + d[:, None], conj, nonfinite), ba)
    rb = to_world(quat_at(T, Q, tb[None, :] + d[:, None], conj, nonfinite), bb)
    m = ((ra[1] * rb[2]) - (ra[2] * rb[1]), (ra[2] * rb[0]) - (ra[0] * rb[2]), (ra[0] * rb[1]) - (ra[1] * rb[0]))
    t = smallest(moments(m), cfg.sweeps)
    best = score(cfg, m, t)
    if n >= 2:
        for h in range(1, cfg.hypotheses + 1):
            i, j = (7 * h) % n, (13 * h + 5) % n
            assert 0 <= i < n and 0 <= j < n
            a, b = [x[:, i] for x in m], [x[:, j] for x in m]
            c = [(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])]
            len2 = ((c[0] * c[0]) + (c[1] * c[1])) + (c[2] * c[2])
            go = len2 > 0.0
            ln = np.sqrt(np.where(go, len2, 1.0))
            th = np.stack([c[0] / ln, c[1] / ln, c[2] / ln], axis=1)
            s = score(cfg, m, th)
            take = go & (s < best)
            best, t = np.where(take, s, best), np.where(take[:, None], th, t)
    for _ in range(cfg.refits):
        x2 = residual2(cfg, m, t)
        w = 1.0 / ((1.0 + x2) * (1.0 + x2))
        t = smallest(moments(m, w), cfg.sweeps)
    cost = score(cfg, m, t)
    assert nonfinite or (np.isfinite(cost).all() and np.isfinite(t).all())
    return (cost, t) if directions else cost


def range_costs(cfg, T, Q, prepared_pairs, delays, conj=False, nonfinite=False):
    """-> (per pair [C][n_pairs], range sum [C])"""
    d = np.asarray(delays, dtype=np.float64).reshape(-1)
    per = np.zeros((len(d), len(prepared_pairs)))
    total = np.zeros(len(d))
    for p, pr in enumerate(prepared_pairs):
        per[:, p] = pair_costs(cfg, T, Q, pr, d, conj, nonfinite=nonfinite)
        total = total + per[:, p]
    return per, total


def round0_count(radius_s, step_s):
    return 2 * int(np.floor(radius_s / step_s)) + 1


def candidates_total(cfg, radius_s):
    return round0_count(radius_s, cfg.step_s) + (cfg.rounds - 1) * LATER


def first_min(costs):
    """the first minimum among the costs that are not NaN; 0 where every cost is NaN"""
    k = -1
    for i in range(len(costs)):
        if costs[i] == costs[i] and (k < 0 or costs[i] < costs[k]):
            k = i
    return max(k, 0)


def search_range(cfg, T, Q, prepared_pairs, initial_delay_s, radius_s, conj=False, nonfinite=False):
    """full_sync of one range -> dict(found, n_coarse, coarse_value, coarse_cost, value, cost, candidates [total], costs [total])"""
    n0 = round0_count(radius_s, cfg.step_s)
    h = (n0 - 1) // 2
    total = candidates_total(cfg, radius_s)
    out = dict(found=0, n_coarse=n0, coarse_value=0.0, coarse_cost=0.0, value=0.0, cost=0.0, candidates=np.zeros(total), costs=np.zeros(total))
    if not prepared_pairs:
        return out
    step = cfg.step_s
    cand = float(initial_delay_s) + ((np.arange(n0) - h).astype(np.float64) * step)
    at = 0
    for rnd in range(cfg.rounds):
        _, costs = range_costs(cfg, T, Q, prepared_pairs, cand, conj, nonfinite)
        k = first_min(costs)
        out["candidates"][at:at + len(cand)], out["costs"][at:at + len(cand)] = cand, costs
        at += len(cand)
        if rnd == 0:
            out.update(found=1, coarse_value=float(cand[k]), coarse_cost=float(costs[k]))
        if rnd == cfg.rounds - 1:
            value = cand[k]
            if cfg.refine and 0 < k < len(cand) - 1:
                den = (costs[k - 1] - (2.0 * costs[k])) + costs[k + 1]
                if den > 0.0:
                    value = cand[k] + (step * ((0.5 * (costs[k - 1] - costs[k + 1])) / den))
            assert nonfinite or np.isfinite(value)
            out.update(value=float(value), cost=float(costs[k]))
        else:
            step = step / 8.0
            cand = cand[k] + ((np.arange(LATER) - 8).astype(np.float64) * step)
    return out


def search(cam, cfg, track_ts_us, track_wxyz, ranges, initial_delay_s, radius_s, conj=False, nonfinite=False):
    """gfw_sync_rs_search's outputs.  ranges: [[(ts_a_us, ts_b_us, points_a, points_b)]] -> (results int/float rows [n][6], candidates [n][total], costs [n][total])"""
    T, Q = track_seconds(track_ts_us), np.asarray(track_wxyz, dtype=np.float64).reshape(-1, 4)
    total = candidates_total(cfg, radius_s)
    res, cands, costs = [], np.zeros((len(ranges), total)), np.zeros((len(ranges), total))
    for r, pairs in enumerate(ranges):
        prepared = [prepare(cam, cfg, (ta, tb), a, b) for ta, tb, a, b in pairs]
        o = search_range(cfg, T, Q, prepared, initial_delay_s, radius_s, conj, nonfinite)
        res.append((o["found"], o["n_coarse"], o["coarse_value"], o["coarse_cost"], o["value"], o["cost"]))
        cands[r], costs[r] = o["candidates"], o["costs"]
    return res, cands, costs


def costs_of(cam, cfg, track_ts_us, track_wxyz, ranges, candidates, nonfinite=False):
    """gfw_sync_rs_costs' outputs: one array of range costs per range for its candidates (seconds)"""
    T, Q = track_seconds(track_ts_us), np.asarray(track_wxyz, dtype=np.float64).reshape(-1, 4)
    out = []
    for pairs, cand in zip(ranges, candidates):
        prepared = [prepare(cam, cfg, (ta, tb), a, b) for ta, tb, a, b in pairs]
        out.append(range_costs(cfg, T, Q, prepared, cand, nonfinite=nonfinite)[1])
    return out
