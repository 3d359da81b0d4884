"""The gyro-match search's kernels (gyroflow_amd/csrc/gfw_sync_gyro.hip) and the entry points' host staging (gfw_gyro_stage), interpreted on the host
(tests/_emu_sync_gyro.py), against the numpy statement (tests/_syncgyrostmt.py): costs, picks, fine candidates and fine costs to the bit, on the smallest shapes
at which the kernel can go wrong.  Bit equality is the whole bound: the arithmetic is f64 and a candidate's sum is the reference's sequential fold."""
import numpy as np
import pytest

import _emu_sync_gyro as E
import _syncgyrostmt as G

F64_MAX = G.F64_MAX


same_bits, make_range = G.same_bits, G.make_range


def check_search(ranges, initial, size):
    """the interpreted search of all `ranges` in one call against the statement's search of each -> (results, coarse costs)"""
    res, coarse, fine, fine_costs, kept = E.sync_gyro_search(ranges, initial, size)
    assert len(res) == len(ranges)
    for i, (est, est_has, gyro, gyro_has) in enumerate(ranges):
        s = G.search(est, est_has, gyro, gyro_has, initial, size)
        r = res[i]
        assert kept[i] == len(G.Tree(gyro, gyro_has).keys), i
        assert (r.found, r.n_coarse) == (s["found"], s["n_coarse"]), (i, r.found, r.n_coarse)
        assert same_bits(coarse[i], s["coarse_costs"]), i
        if not s["found"]:
            assert np.all(fine_costs[i] == 0.0)                                    # the second stage does nothing
            continue
        assert same_bits([r.coarse_value, r.coarse_cost, r.value, r.cost], [s["coarse_value"], s["coarse_cost"], s["value"], s["cost"]]), (i, r.coarse_value, r.value, s["coarse_value"], s["value"])
        assert same_bits(fine[i], s["fine"]) and same_bits(fine_costs[i], s["fine_costs"]), i
    return res, coarse


@pytest.mark.parametrize("n_est", [1, 2, 3, 130])
@pytest.mark.parametrize("n_gyro", [1, 2, 3000])
def test_sample_counts(n_est, n_gyro):
    res, coarse = check_search([make_range(n_est, n_gyro, seed=n_est)], 0.0, 40.0)
    assert res[0].found == 1 and res[0].n_coarse == 80
    if n_gyro == 3000:
        assert res[0].cost < F64_MAX and abs(res[0].value - 12.3) <= 2.0           # the planted delay (1 kHz gyro: 1 ms + 1 ms)


def test_two_samples_with_one_match_are_refused_three_with_two_are_accepted():
    est, _, gyro, _ = make_range(2, 3000, seed=7)
    cands = [np.array([0.0, 12.0, -3.5])]
    assert np.all(E.sync_gyro_costs([(est, [1, 0], gyro, None)], cands)[0] == F64_MAX)                      # 1 > 2 / 2 is false
    assert np.all(E.sync_gyro_costs([(est, [1, 1], gyro, None)], cands)[0] < F64_MAX)
    est3 = make_range(3, 3000, seed=7)[0]
    got = E.sync_gyro_costs([(est3, [1, 0, 1], gyro, None)], cands)[0]                                     # 2 > 3 / 2
    assert np.all(got < F64_MAX) and same_bits(got, G.costs(cands[0], est3, [1, 0, 1], G.Tree(gyro)))
    assert np.all(E.sync_gyro_costs([(est3, [0, 0, 1], gyro, None)], cands)[0] == F64_MAX)


def test_duplicate_keys_the_later_sample_wins_and_a_descending_slice():
    est, _, gyro, _ = make_range(40, 600, seed=3)
    dup = np.concatenate([gyro, gyro[100:300] + np.array([0.0001, 50.0, -20.0, 5.0])])                      # the same microsecond keys (0.1 us later), other values, given later
    assert len(G.Tree(dup).keys) == 600
    has = np.ones(len(dup), dtype=np.uint8)
    has[150] = 0                                                                                           # the replaced sample's None does not survive ...
    has[600 + 60] = 0                                                                                      # ... the replacing sample's does
    r_dup = (est, None, dup, has)
    r_desc = (est, None, gyro[::-1].copy(), None)
    r_plain = (est, None, gyro, None)
    res, coarse = check_search([r_dup, r_desc, r_plain], 10.0, 30.0)
    assert same_bits(coarse[1], coarse[2]) and bytes(res[1]) == bytes(res[2])                               # the order of a slice does not matter
    assert not same_bits(coarse[0], coarse[2])
    shuffled = dup[np.random.RandomState(1).permutation(600)]                                              # (the first 600: distinct keys)
    assert same_bits(E.sync_gyro_costs([(est, None, shuffled, None)], [[3.0, 12.0]])[0], E.sync_gyro_costs([(est, None, dup[:600], None)], [[3.0, 12.0]])[0])


def test_none_entries_on_either_side():
    est, _, gyro, _ = make_range(60, 2000, seed=4)
    est_has = np.ones(60, dtype=np.uint8)
    est_has[[0, 7, 8, 59]] = 0
    gyro_has = np.ones(2000, dtype=np.uint8)
    gyro_has[::3] = 0                                                                                      # a hit on a None is no match: the lookup does not move on
    res, coarse = check_search([(est, est_has, gyro, gyro_has), (est, est_has, gyro, None), (est, None, gyro, gyro_has)], 0.0, 25.0)
    assert len({coarse[k].tobytes() for k in range(3)}) == 3
    all_none = check_search([(est, np.zeros(60, dtype=np.uint8), gyro, None), (est, None, gyro, np.zeros(2000, dtype=np.uint8))], 0.0, 25.0)[1]
    assert np.all(all_none == F64_MAX)


def test_queries_that_go_negative_and_past_the_end_inside_one_sweep():
    """gyro samples from 100 ms to 400 ms, estimated samples from 180 ms: over candidates -300 .. 299 the queries run from below zero (they land on the first
    sample: a match) to past the last key (a miss)"""
    est, _, gyro, _ = make_range(8, 301, seed=5, start_ms=180.0, gyro_from_ms=100.0, fps=50.0)
    res, coarse = check_search([(est, None, gyro, None)], 0.0, 300.0)
    c = coarse[0]
    assert c[0] == F64_MAX and c[-1] < F64_MAX                                                              # offset -300: every query past the end; +299: every query negative
    assert same_bits(c[-1], c[-20])                                                                        # ... all of them on the first sample: one cost
    assert 0 < np.sum(c == F64_MAX) < len(c)


@pytest.mark.parametrize("size,n_coarse", [(0.0, 0), (0.9, 0), (2.5, 4), (300.0, 600)])
def test_search_sizes(size, n_coarse):
    res, coarse = check_search([make_range(20, 800, seed=6)], 5.0, size)
    assert res[0].n_coarse == n_coarse and res[0].found == (1 if n_coarse else 0) and coarse.shape == (1, n_coarse)
    if size == 2.5:
        assert same_bits(G.coarse_candidates(5.0, 2.5), [2.5, 3.5, 4.5, 5.5])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_candidate_counts_around_a_wave_and_a_workgroup(n):
    est, _, gyro, _ = make_range(9, 500, seed=8)
    cands = np.random.RandomState(n).uniform(-200.0, 200.0, n)
    got = E.sync_gyro_costs([(est, None, gyro, None)], [cands])[0]
    assert same_bits(got, G.costs(cands, est, None, G.Tree(gyro)))
    assert got[0] == G.cost_scalar(float(cands[0]), est, None, G.Tree(gyro)) and got[-1] == G.cost_scalar(float(cands[-1]), est, None, G.Tree(gyro))


def test_a_plateau_of_equal_costs_the_last_candidate_wins():
    """a gyro sampled every 100 ms: neighbouring candidates hit the same samples and cost the same"""
    est, _, gyro, _ = make_range(4, 60, seed=9, rate=10.0, fps=2.5)
    res, coarse = check_search([(est, None, gyro, None)], 0.0, 150.0)
    c = coarse[0]
    low = np.min(c)
    at = np.flatnonzero(c == low)
    assert len(at) > 1                                                                                     # a plateau
    assert res[0].coarse_value == float(G.coarse_candidates(0.0, 150.0)[at[-1]])
    fine_c = G.costs(G.fine_candidates(res[0].coarse_value), est, None, G.Tree(gyro))
    fat = np.flatnonzero(fine_c == np.min(fine_c))
    assert len(fat) > 1 and res[0].value == float(G.fine_candidates(res[0].coarse_value)[fat[-1]])


def test_every_cost_is_f64_max_the_last_candidate_wins():
    est, _, gyro, _ = make_range(10, 50, seed=10, gyro_from_ms=-90000.0)                                    # every query past the end
    res, coarse = check_search([(est, None, gyro, None)], 0.0, 70.0)
    assert np.all(coarse == F64_MAX)
    r = res[0]
    assert r.found == 1 and r.coarse_value == 69.0 and r.coarse_cost == F64_MAX
    assert r.value == float(G.fine_candidates(69.0)[-1]) and r.cost == F64_MAX
    no_gyro = check_search([(est, None, np.zeros((0, 4)), None)], 0.0, 3.0)[0][0]
    assert no_gyro.found == 1 and no_gyro.coarse_value == 2.0 and no_gyro.cost == F64_MAX


def test_five_ranges_in_one_call_equal_their_own_calls():
    ranges = [make_range(130, 3000, seed=11), make_range(1, 2, seed=12), make_range(0, 40, seed=13), make_range(33, 700, seed=14, rate=200.0, offset_ms=-31.7),
              make_range(3, 1, seed=15)]
    res, coarse = check_search(ranges, -4.0, 140.0)
    assert np.all(coarse[2] == F64_MAX) and res[2].found == 1                                               # a range without samples: `!of.is_empty()` fails
    for i, r in enumerate(ranges):
        one, c1, f1, fc1, _ = E.sync_gyro_search([r], -4.0, 140.0)
        assert bytes(one[0]) == bytes(res[i]) and same_bits(c1[0], coarse[i]), i
    cands = [np.linspace(-50.0, 50.0, k) for k in (300, 1, 0, 257, 64)]                                      # caller-given candidates, another count per range
    got = E.sync_gyro_costs(ranges, cands)
    for i, (est, eh, gyro, gh) in enumerate(ranges):
        assert same_bits(got[i], G.costs(cands[i], est, eh, G.Tree(gyro, gh))), i


def test_slices_that_start_inside_their_arrays():
    """est_first[0], gyro_first[0] and cand_first[0] above 0: a range owns its first .. entries of every array, and of `costs` the same entries as of `candidates` —
    what lies in front belongs to no range: not read, not written"""
    ranges = [make_range(33, 700, seed=14, rate=200.0, offset_ms=-31.7), make_range(0, 40, seed=13), make_range(5, 300, seed=16)]
    cands = [np.linspace(-50.0, 50.0, k) for k in (70, 3, 260)]
    plain = E.sync_gyro_costs(ranges, cands)
    for lead in ((0, 0, 9), (4, 0, 0), (0, 6, 0), (5, 7, 300)):
        per, whole = E.sync_gyro_costs(ranges, cands, lead=lead, whole=True)
        assert len(whole) == 333 + lead[2] and np.all(whole[:lead[2]] == -7.0), lead                       # the entries in front of cand_first[0] are nobody's
        for i in range(3):
            assert same_bits(per[i], plain[i]), (lead, i)
            assert same_bits(per[i], G.costs(cands[i], ranges[i][0], ranges[i][1], G.Tree(ranges[i][2], ranges[i][3]))), (lead, i)
    res0, coarse0, fine0, fc0, _ = E.sync_gyro_search(ranges, -4.0, 140.0)
    res1, coarse1, fine1, fc1, _ = E.sync_gyro_search(ranges, -4.0, 140.0, lead=(5, 7, 0))
    assert [bytes(r) for r in res0] == [bytes(r) for r in res1] and same_bits(coarse0, coarse1) and same_bits(fc0, fc1)
