"""gfw_sync_rs_search's and gfw_sync_rs_costs' kernels (gyroflow_amd/csrc/gfw_sync_rs.hip) interpreted on the host (tests/_emu_rs_sync.py) against the f64 statement
(tests/_rssyncstmt.py): results, every round's candidates and range costs, bit for bit, on the "emu" shape of tests/_rssynccase.py — 2 ranges of 3 small pairs
(5, 66, 9 and 12, 1, 70 points: under, over and at one point of a wave), radius 6 ms: 5 + 3 x 17 candidates — with every array of the work space against an
inaccessible page, at its end and at its start.  The statement's result is computed once and shared."""
import numpy as np
import pytest

import _emu_rs_sync as ER
import _pairbase as PB
import _rssynccase as RC
import _rssyncstmt as RS


def run(c, **kw):
    cam = c.cam
    return ER.sync_rs_search(cam.kp, cam.clip.model, cam.clip.digital, RC.cfg_of(cam, c.cfg), c.ranges, c.track[0], c.track[1], c.initial_s, c.radius_s, **kw)


@pytest.mark.parametrize("guard", [1, 2])
def test_interpreted_kernels_equal_the_statement_to_the_bit(guard):
    c = RC.case("emu-pinhole")
    RC.assert_search_equal(run(c, guard=guard), c.statement, "emu-pinhole guard %d" % guard)
    assert [r[:2] for r in c.statement[0]] == [(1, 5), (1, 5)] and c.statement[1].shape == (2, 5 + 3 * 17)


def test_the_case_is_not_degenerate():
    """the rounds move the pick, the parabola moves the final delay off the last pick, and the costs differ between candidates (a later round repeats its
    centre and the two candidates a former step away: at most 3 of its 17 costs were seen before)"""
    res, cand, cost = RC.case("emu-pinhole").statement
    for r, row in enumerate(res):
        assert row[4] != row[2] and row[5] < row[3] and len(set(cost[r].tolist())) >= 5 + 3 * 14
        assert row[4] not in cand[r].tolist()


def test_without_round_outputs_the_work_space_serves_and_costs_equal_the_searchs():
    c = RC.case("emu-pinhole")
    cam = c.cam
    got = run(c, rounds=False)
    RC.assert_search_equal((got[0], c.statement[1], c.statement[2]), c.statement, "emu-pinhole without round outputs")
    assert (got[1] == -7.0).all() and (got[2] == -7.0).all()
    cands = [c.statement[1][0][:7], c.statement[1][1][3:6]]
    costs = ER.sync_rs_costs(cam.kp, cam.clip.model, cam.clip.digital, RC.cfg_of(cam, c.cfg), c.ranges, c.track[0], c.track[1], cands)
    assert (RC.bits(costs[0]) == RC.bits(c.statement[2][0][:7])).all() and (RC.bits(costs[1]) == RC.bits(c.statement[2][1][3:6])).all()


def test_the_entry_points_check_names_the_range_or_pair():
    c = RC.case("emu-pinhole")
    cam = c.cam
    args = (cam.kp, cam.clip.model, cam.clip.digital, RC.cfg_of(cam, c.cfg))
    with pytest.raises(ER.Refused, match="track sample 3: timestamp"):
        ts = c.track[0].copy(); ts[3] = ts[2]
        ER.sync_rs_search(*args, c.ranges, ts, c.track[1], c.initial_s, c.radius_s)
    with pytest.raises(ER.Refused, match="a track of 1 samples"):
        ER.sync_rs_search(*args, c.ranges, c.track[0][:1], c.track[1][:1], c.initial_s, c.radius_s)
    big = [[(0, 1, np.zeros((4097, 2), dtype=np.float32), np.zeros((4097, 2), dtype=np.float32))]]
    with pytest.raises(ER.Refused, match="pair 0: 4097 points, at most 4096"):
        ER.sync_rs_search(*args, big, c.track[0], c.track[1], c.initial_s, c.radius_s)
    with pytest.raises(ER.Refused, match="radius"):
        ER.sync_rs_search(*args, c.ranges, c.track[0], c.track[1], c.initial_s, -1.0)
    cfg = RC.cfg_of(cam, c.cfg); cfg.rounds = 9
    with pytest.raises(ER.Refused, match="9 rounds, 1 .. 8"):
        ER.sync_rs_search(cam.kp, cam.clip.model, cam.clip.digital, cfg, c.ranges, c.track[0], c.track[1], c.initial_s, c.radius_s)


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged from 0 and the points from the third on (tests/_pairbase.py)"""
    c = PB.rs_sync()
    cam = c.cam
    args = (cam.kp, cam.clip.model, cam.clip.digital, RC.cfg_of(cam, c.cfg), c.ranges, c.track[0], c.track[1])
    costs = PB.assert_base_does_not_matter(lambda: ER.sync_rs_costs(*args, c.candidates), "sync_rs_costs")
    assert len(costs[0]) == 3 and len(set(costs[0].tolist())) == 3 and all(v > 0.0 for v in costs[0])
    rows, cand, cost = PB.assert_base_does_not_matter(lambda: tuple(ER.sync_rs_search(*args, c.initial_s, c.radius_s)), "sync_rs_search")
    assert cand.shape == (1, 3) and rows[0][1] == 3 and len(set(cost[0].tolist())) == 3
