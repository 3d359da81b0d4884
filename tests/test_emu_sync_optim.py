"""The sync-point choice's kernels (gyroflow_amd/csrc/gfw_sync_optim.hip) and the entry points' host arithmetic (gfw_sync_optim_host.h), interpreted on the host
(tests/_emu_sync_optim.py), against the f32 statement (tests/_syncoptimstmt.py): band energies, rank, masked rank, suppressed rank and points to the bit, on the
smallest shapes at which the kernels can go wrong.  Bit equality is the whole bound: a bin is a sequential f32 fold whatever the launch shape."""
import math

import numpy as np
import pytest

import _emu_sync_optim as E
import _syncoptimstmt as S

KEYS = ("lf", "mf", "hf", "rank", "masked", "rank_nms", "points")


def noise(n, seed, scale=30.0):
    return np.random.RandomState(seed).normal(0.0, scale, (3, n))


def tone(n, rate, freq, amp, seed=0, noise_scale=0.0):
    t = np.arange(n) / rate
    g = np.stack([amp * np.sin(2.0 * math.pi * freq * t + a * 2.0 * math.pi / 3.0) for a in range(3)])
    return g + (noise(n, seed, noise_scale) if noise_scale else 0.0)


def check(gyro, rate, target, trims=((0.0, 1e9),)):
    e = E.run(gyro, rate, target, trims)
    s = S.run_f32(gyro, rate, target, trims)
    n = S.fft_size(rate)
    assert list(e["shape"]) == [n, S.n_windows(np.asarray(gyro).reshape(3, -1).shape[1], n), S.as_usize(rate / 16.0 / 2.0 * 8.0), (len(s["rank"]) + target - 1) // target] + S.band_bins(n, rate)
    for k in KEYS:
        assert S.same_bits(e[k], s[k]), (k, e[k][:4], s[k][:4])
    return e


@pytest.mark.parametrize("rate,windows", [(16.0, 3), (97.3, 5), (200.0, 4), (520.0, 8)])
def test_fft_sizes_odd_below_a_workgroup_and_above_it(rate, windows):
    """16: the smallest; 97: odd (N/2 = 48, the mirror index N-1-k); 200: 101 bins in a workgroup of 256; 520: 261 bins — a lane owns two, and the pair sum crosses a round"""
    n = S.fft_size(rate)
    e = check(noise(n + 16 * (windows - 1) + 7, int(rate)), rate, 2)
    assert len(e["rank"]) == windows and np.all(e["mf"] > 0.0)


@pytest.mark.parametrize("extra,windows", [(-1, 0), (0, 1), (15, 1), (16, 2)])
def test_window_counts_at_the_edges(extra, windows):
    e = check(noise(32 + extra, 1), 32.0, 3)
    assert len(e["rank"]) == windows
    if not windows:
        assert len(e["points"]) == 0


def test_one_window_more_than_a_workgroup_of_windows_and_of_segments():
    """257 windows: the rank and suppression stages tile by 256; one segment of 257 windows: a lane of the pick stage folds two; 300 segments: a lane of the gather
    stage owns two"""
    g = tone(16 + 16 * 256, 16.0, 3.0, 40.0, seed=2, noise_scale=8.0)
    for target in (1, 2, 300):
        e = check(g, 16.0, target, [(0.0, 1e9)])
        assert len(e["rank"]) == 257
    assert len(e["points"]) > 2


def test_the_largest_fft_size():
    e = check(noise(8192, 5), 8192.0, 1)
    assert len(e["rank"]) == 1 and list(e["shape"][4:]) == [0, 2, 30, 2000]


def test_band_ends_at_50_hz_and_a_rate_whose_hf_ends_at_the_last_bin():
    e = check(noise(50 + 40, 6), 50.0, 1)
    assert np.all(e["hf"] == 0.0) and list(e["shape"][4:]) == [0, 2, 24, 24]
    e = check(noise(4000, 7), 4000.0, 1)
    assert list(e["shape"][4:]) == [0, 2, 30, 1999]


def test_low_motion_zero_and_the_penalties():
    e = check(noise(50 * 5, 8, scale=0.05), 50.0, 2)
    assert e["mf"].max() < 50.0 and len(e["points"]) == 0                                # (lf + mf): the other formula
    e = check(np.zeros((3, 200)), 50.0, 3)
    assert np.all(e["rank"] == 0.0) and len(e["points"]) == 0
    loud = tone(400, 100.0, 40.0, 4000.0) + tone(400, 100.0, 0.7, 9000.0) + tone(400, 100.0, 9.0, 60.0)
    e = check(loud, 100.0, 2)
    assert e["hf"].min() > 450.0 and e["lf"].min() > 650.0                               # both nlfunc terms are live


@pytest.mark.parametrize("windows,rule", [(119, False), (121, True)])
def test_the_two_second_rule(windows, rule):
    g = tone(160 + 16 * (windows - 1), 160.0, 8.0, 50.0, seed=9, noise_scale=2.0)
    e = check(g, 160.0, 3)
    assert (e["masked"][0] == 0.0) == rule and (e["masked"][-1] == 0.0) == rule and np.all(e["rank"] > 50.0)


def test_trim_ranges_none_outside_and_two_disjoint():
    g = tone(160 + 16 * 59, 160.0, 8.0, 50.0, seed=10, noise_scale=2.0)
    assert len(check(g, 160.0, 2, [])["points"]) == 0
    assert len(check(g, 160.0, 2, [(100.0, 200.0)])["points"]) == 0
    e = check(g, 160.0, 2, [(1.0, 1.5), (5.5, 5.7)])                                      # 40 windows apart: beyond the suppression radius
    assert 8 <= np.count_nonzero(e["masked"]) <= 9 and len(e["points"]) == 2


def test_more_segments_than_windows_and_a_plateau_of_equal_ranks():
    """a tone whose period divides the hop: every window holds the same samples, every rank is the same number — nothing is suppressed, and of the equal maxima of
    a segment the last wins"""
    g = tone(32 + 16 * 9, 32.0, 4.0, 50.0)
    e = check(g, 32.0, 3)
    assert len(set(e["rank"].tolist())) == 1 and e["rank"][0] > 50.0 and np.all(e["rank_nms"] == e["rank"])
    assert list(e["points"]) == [(i * 16.0 + 16.0) / 32.0 * 1000.0 for i in (3, 7, 9)]
    e = check(g, 32.0, 14)                                                              # segments of one window: 10 points, four segments beyond the end
    assert len(e["points"]) == 10


def test_the_last_element_survives_the_suppression():
    t = np.arange(32 + 16 * 5) / 32.0
    g = tone(len(t), 32.0, 5.0, 90.0) * np.exp(-t / 2.0)                                # decays: every window ranks below the one before
    e = check(g, 32.0, 2)
    assert np.all(np.diff(e["rank"]) < 0.0) and e["rank"][-1] > 50.0
    assert e["rank_nms"][0] == e["rank"][0] and np.all(e["rank_nms"][1:-1] == 0.0) and e["rank_nms"][-1] == e["rank"][-1]
    assert len(e["points"]) == 2


def test_the_rank_entry_runs_the_first_three_stages_only():
    g = noise(200 + 16 * 3, 11)
    e = E.run(g, 200.0, points=False)
    s = S.run_f32(g, 200.0, 1, [(0.0, 1e9)])
    for k in ("lf", "mf", "hf", "rank"):
        assert S.same_bits(e[k], s[k]), k
    assert np.all(e["rank_nms"] == -7.0)                                                 # not written


def test_a_planted_clip_end_to_end():
    g, centres = S.planted_clip(97.3, 45.0)
    e = check(g, 97.3, 4, [(0.0, 45.0)])
    assert len(e["points"]) >= 3
