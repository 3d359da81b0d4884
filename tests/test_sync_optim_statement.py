"""The numpy statements of OptimSync::run (tests/_syncoptimstmt.py) held to their purpose — planted bursts are found — and to one another: the f32 form, which the
device computes to the bit, against the literal f64 form within a bound derived from the number formats alone (the statement's docstring); and the literal form's
edge cases against the reference's own loops, transliterated below."""
import math

import numpy as np
import pytest

import _syncoptimstmt as S

_clips = {}


def clip(i):
    """(gyro, burst centres, rate, duration, literal result, f32 result) of planted clip i, computed once"""
    if i not in _clips:
        rate, dur = S.PLANTED[i]
        g, centres = S.planted_clip(rate, dur)
        _clips[i] = (g, centres, rate, dur, S.run_literal(g, rate, 4, [(0.0, dur)]), S.run_f32(g, rate, 4, [(0.0, dur)]))
    return _clips[i]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_planted_bursts_are_found_by_both_forms(i):
    """Both forms pick the same points, and every burst inside the clip has a point within two hops of 16 samples.  (Seed 0 of the generator; see planted_clip for
    how much of that is the draw.)"""
    g, centres, rate, dur, lit, f32 = clip(i)
    assert len(centres) == (4, 3, 2)[i]
    assert S.same_bits(lit["points"], f32["points"]), (lit["points"], f32["points"])
    assert len(lit["points"]) >= len(centres)
    hop_ms = 16.0 / rate * 1000.0
    for c in centres:
        d = float(np.min(np.abs(lit["points"] - c * 1000.0)))
        print("rate %g: burst at %g s, nearest point %.1f ms away (hop %.1f ms)" % (rate, c, d, hop_ms))
        assert d <= 2.0 * hop_ms, (rate, c, d, hop_ms)
    assert lit["ratio"] == 16.0 / rate and f32["ratio"] == lit["ratio"]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_band_energies_of_the_f32_form_lie_within_the_derived_bound(i):
    g, centres, rate, dur, lit, f32 = clip(i)
    bound = S.band_bound(lit["merged"], lit["absum"], rate)
    assert bound.shape == (3, len(lit["mf"])) and len(lit["mf"]) > 100
    for b, name in enumerate(("lf", "mf", "hf")):
        diff = np.abs(f32[name].astype(np.float64) - lit[name])
        print("rate %g %s: max |f32 - f64| %.3g, smallest bound %.3g, largest value %.6g" % (rate, name, diff.max(), bound[b].min(), lit[name].max()))
        assert np.all(bound[b] > 0.0) and np.all(diff < bound[b]), (name, float(np.max(diff / bound[b])))
    # the bound is no licence: it stays below a thousandth of the largest mid-band energy
    assert bound[1].max() < 1e-3 * lit["mf"].max()


# ---- the reference's loops (:151-204), transliterated: what `tail` is held to ----
def reference_loops(rank, sample_rate, n, target, trims):
    rank = [float(v) for v in rank]
    ratio = 16.0 / sample_rate
    for i in range(len(rank)):
        time = i * ratio
        if rank[i] < 50.0 or not any(time >= a and time <= b for a, b in trims):
            rank[i] = 0.0
    total = len(rank) * ratio
    if total > 12.0:
        for i in range(len(rank)):
            time = i * ratio
            if time < 2.0 or time >= (total - 2.0):
                rank[i] = 0.0
    radius = int((sample_rate / 16.0 / 2.0) * 8.0)
    nms = list(rank)
    for i in range(len(rank)):
        for j in range(max(i - radius, 0), min(i + radius, len(rank) - 1)):
            if rank[j] < rank[i]:
                nms[j] = 0.0
    seg = (len(nms) + target - 1) // target
    points = []
    for i in range(target):
        start = i * seg
        end = min(start + seg, len(nms))
        if start > end or end > len(nms) or start == end:
            continue
        best = start
        for c in range(start, end):
            if not (nms[best] > nms[c]):                                               # Iterator::max_by: the last maximal element
                best = c
        if nms[best] < 0.1:
            continue
        points.append((best * 16.0 + n / 2.0) / sample_rate * 1000.0)
    return points, rank, nms


def f32_max(a, b):
    """f32::max: the other operand when one is a NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def reference_from_bands(lf, mf, hf, sample_rate, n, target, trims):
    """The `mf_max` fold and the rank formulas (:136-149) in f32, one scalar operation at a time, ahead of reference_loops (whose compares are exact on f32 values
    held as Python floats) -> (points, rank, masked rank, suppressed rank, low_motion)"""
    T = np.float32
    nlfunc = lambda arg, trip: T(0.0) if arg < trip else arg - trip
    mf_max = T(0.0)
    for v in mf:
        mf_max = f32_max(mf_max, T(v))
    low_motion = bool(mf_max < T(50.0))
    rank = []
    with np.errstate(all="ignore"):
        for l, m, h in zip(lf, mf, hf):
            l, m, h = T(l), T(m), T(h)
            if low_motion:
                rank.append((l + m) / (T(1.0) + nlfunc(h, T(450.0)) * T(0.003)))
            else:
                rank.append(m / (T(1.0) + nlfunc(h, T(450.0)) * T(0.003)) / (T(1.0) + nlfunc(l, T(650.0)) * T(0.003)))
    assert all(type(v) is T for v in rank)
    pts, masked, nms = reference_loops(rank, sample_rate, n, target, trims)
    return np.array(pts, dtype=np.float64), np.array(rank, dtype=T), np.array(masked, dtype=T), np.array(nms, dtype=T), low_motion


def tail64(mf, sample_rate, target, trims, lf=None, hf=None):
    mf = np.asarray(mf, dtype=np.float64)
    z = np.zeros_like(mf)
    return S.tail(z if lf is None else np.asarray(lf, dtype=np.float64), mf, z if hf is None else np.asarray(hf, dtype=np.float64), sample_rate,
                  S.fft_size(sample_rate), target, trims, np.float64)


@pytest.mark.parametrize("seed", range(6))
def test_masks_nms_and_picks_equal_the_reference_loops(seed):
    rs = np.random.RandomState(seed)
    w = int(rs.randint(1, 140))
    rate = float(rs.choice([32.0, 50.0, 97.3, 160.0]))
    mf = np.round(rs.uniform(0.0, 200.0, w))                                           # rounded: ties happen
    trims = [(0.5, 4.0), (6.0, 9.0)] if seed % 2 else [(0.0, 1e9)]
    for target in (1, 3, w, w + 5):
        t = tail64(mf, rate, target, trims)
        pts, masked, nms = reference_loops(t["rank"], rate, S.fft_size(rate), target, trims)
        assert np.array_equal(t["masked"], masked) and np.array_equal(t["rank_nms"], nms)
        assert np.array_equal(t["points"], pts), (w, rate, target)
    assert np.array_equal(t["rank"], mf)                                               # hf < 450, lf < 650: the rank is mf


@pytest.mark.parametrize("extra,windows", [(-1, 0), (0, 1), (15, 1), (16, 2)])
def test_window_counts_at_the_edges(extra, windows):
    n = 32
    g = np.random.RandomState(3).normal(0.0, 30.0, (3, n + extra))
    r = S.run_literal(g, 32.0, 2, [(0.0, 100.0)])
    f = S.run_f32(g, 32.0, 2, [(0.0, 100.0)])
    assert len(r["rank"]) == windows == len(f["rank"]) and r["merged"].shape == (windows, 16)
    if windows == 0:
        assert len(r["points"]) == 0 and len(f["points"]) == 0


def test_band_ends_clamp_at_low_and_high_rates():
    assert S.band_bins(50, 50.0) == [0, 2, 24, 24]                                      # 30 Hz and 2000 Hz clamp to N/2 - 1: hf is empty
    assert S.band_bins(4000, 4000.0) == [0, 2, 30, 1999]                                # hf ends at N/2 - 1, exclusive: that bin is in no band
    assert S.band_bins(200, 200.0) == [0, 2, 30, 99]
    assert S.band_bins(97, 97.3) == [0, 2, 30, 47]
    g = np.random.RandomState(4).normal(0.0, 30.0, (3, 50 + 16))
    r = S.run_literal(g, 50.0, 1, [(0.0, 100.0)])
    assert np.all(r["hf"] == 0.0) and np.all(r["mf"] > 0.0)
    g = np.random.RandomState(5).normal(0.0, 30.0, (3, 4000))
    r = S.run_literal(g, 4000.0, 1, [(0.0, 100.0)])
    assert np.allclose(r["hf"], np.sum(r["merged"][:, 30:1999], axis=1), rtol=1e-12) and r["merged"][0, 1999] > 0.0


def test_low_motion_takes_the_other_rank_formula():
    mf, lf, hf = np.array([10.0, 49.0, 30.0]), np.array([100.0, 700.0, 5.0]), np.array([0.0, 500.0, 0.0])
    t = tail64(mf, 50.0, 1, [(0.0, 100.0)], lf=lf, hf=hf)
    assert np.array_equal(t["rank"], (lf + mf) / (1.0 + np.array([0.0, 50.0, 0.0]) * 0.003))
    t = tail64(np.array([10.0, 50.0, 30.0]), 50.0, 1, [(0.0, 100.0)], lf=lf, hf=hf)      # max(mf) = 50 is not < 50
    want = np.array([10.0, 50.0, 30.0]) / (1.0 + np.array([0.0, 50.0, 0.0]) * 0.003) / (1.0 + np.array([0.0, 50.0, 0.0]) * 0.003)
    assert np.array_equal(t["rank"], want)
    quiet = np.random.RandomState(6).normal(0.0, 0.05, (3, 50 * 6))                      # a clip that hardly moves
    r = S.run_literal(quiet, 50.0, 2, [(0.0, 100.0)])
    assert r["mf"].max() < 50.0 and np.array_equal(r["rank"], (r["lf"] + r["mf"]) / 1.0) and len(r["points"]) == 0


def test_an_all_zero_gyro_ranks_zero_and_yields_nothing():
    for run in (S.run_literal, S.run_f32):
        r = run(np.zeros((3, 200)), 50.0, 3, [(0.0, 100.0)])
        assert len(r["rank"]) == 10 and np.all(r["rank"] == 0.0) and np.all(r["rank_nms"] == 0.0) and len(r["points"]) == 0


@pytest.mark.parametrize("windows,rule", [(119, False), (121, True)])
def test_the_two_second_rule_at_11_9_and_12_1_seconds(windows, rule):
    rate = 160.0                                                                        # ratio 0.1 s: 119 windows span 11.9 s, 121 span 12.1 s
    mf = np.full(windows, 100.0)
    t = tail64(mf, rate, 1, [(0.0, 100.0)])
    assert windows * t["ratio"] == pytest.approx(windows / 10.0)
    if rule:
        time = np.arange(windows) * t["ratio"]
        cleared = (time < 2.0) | (time >= windows * t["ratio"] - 2.0)
        assert np.all(t["masked"][cleared] == 0.0) and np.all(t["masked"][~cleared] == 100.0) and 35 < np.count_nonzero(cleared) < 45
    else:
        assert np.all(t["masked"] == 100.0)


def test_trim_ranges_that_cover_nothing_and_two_disjoint_ones():
    mf = np.full(60, 100.0)
    assert len(tail64(mf, 160.0, 2, [])["points"]) == 0                                  # `any` over nothing
    assert len(tail64(mf, 160.0, 2, [(100.0, 200.0), (-5.0, -1.0)])["points"]) == 0
    t = tail64(mf, 160.0, 2, [(1.0, 1.5), (4.0, 4.2)])
    time = np.arange(60) * 0.1
    inside = ((time >= 1.0) & (time <= 1.5)) | ((time >= 4.0) & (time <= 4.2))
    assert np.array_equal(t["masked"] != 0.0, inside) and 8 <= np.count_nonzero(inside) <= 9
    assert len(t["points"]) == 2


def test_targets_of_one_and_of_more_than_the_windows():
    mf = np.array([60.0, 90.0, 70.0, 0.0, 80.0])
    one = tail64(mf, 32.0, 1, [(0.0, 100.0)])                                            # radius 8: one survivor
    assert list(one["rank_nms"]) == [0.0, 90.0, 0.0, 0.0, 80.0]                          # ... and the last element, which is never cleared
    assert list(one["points"]) == [(1 * 16.0 + 16.0) / 32.0 * 1000.0]
    many = tail64(mf, 32.0, 9, [(0.0, 100.0)])                                           # segments of one window; those starting beyond the end yield nothing
    assert list(many["points"]) == [(1 * 16.0 + 16.0) / 32.0 * 1000.0, (4 * 16.0 + 16.0) / 32.0 * 1000.0]


def test_of_two_equal_maxima_in_a_segment_the_last_wins():
    mf = np.array([60.0, 90.0, 70.0, 90.0, 60.0, 55.0])
    t = tail64(mf, 32.0, 1, [(0.0, 100.0)])
    assert list(t["rank_nms"]) == [0.0, 90.0, 0.0, 90.0, 0.0, 55.0]                      # equal neighbours do not clear one another (`<`)
    assert list(t["points"]) == [(3 * 16.0 + 16.0) / 32.0 * 1000.0]


def test_the_last_element_survives_the_nms():
    mf = np.array([100.0, 90.0, 80.0, 70.0])
    t = tail64(mf, 32.0, 2, [(0.0, 100.0)])
    assert list(t["rank_nms"]) == [100.0, 0.0, 0.0, 70.0]
    assert list(t["points"]) == [16.0 / 32.0 * 1000.0, (3 * 16.0 + 16.0) / 32.0 * 1000.0]
