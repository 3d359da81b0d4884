"""The statement of the rs-sync offset search (tests/_rssyncstmt.py) held to its purpose, on the CPU: it must find the delay planted into clips that an independent
float64 path makes (tests/_rssynccase.py) — every point observed at its own row time, a camera that rotates and moves, outliers — before the device is compared
with it.  Nothing reference-produced exists to compare with: the solver, the rs-sync crate, is not in the reference tree.

The bar of the final delay is one gyro sample period (1 ms at 1 kHz, 5 ms at 200 Hz): the track carries nothing finer.  Measured worst |error| per class
(tests/README_rs_sync.md has the table): clean 1 kHz 0.0009 ms, 30 % outliers 1 kHz 0.0085 ms, clean 200 Hz 0.014 ms, 30 % outliers 200 Hz 0.11 ms."""
import numpy as np
import pytest

import _rssynccase as RC
import _rssyncstmt as RS


def round0(c, **kw):
    res, cands, _ = c.searched(**kw)
    n0 = res[0][1]
    nearest = cands[0][:n0][np.argmin(np.abs(cands[0][:n0] * 1000.0 - c.delay_ms))]
    return res[0], nearest


@pytest.mark.parametrize("name", sorted(RC.CLIPS))
def test_round_0_picks_the_candidate_nearest_the_planted_delay(name):
    c = RC.clip(name)
    r, nearest = round0(c)
    assert r[0] == 1 and r[1] == 21 and r[2] == nearest, (name, r, nearest)


@pytest.mark.parametrize("name", sorted(RC.INSIDE))
def test_the_final_delay_lies_within_one_gyro_sample_period_of_the_truth(name):
    c = RC.clip(name)
    r, _ = round0(c)
    err_ms = abs(r[4] * 1000.0 - c.delay_ms)
    print("%s: |error| %.6f ms, cost %.6g" % (name, err_ms, r[5]))
    assert err_ms < 1000.0 / c.rate_hz, (name, err_ms)
    assert r[5] <= r[3]                                                               # the rounds never raise the cost: the pick is among the next round's candidates


def test_the_delay_outside_the_search_ends_at_the_edge_the_acceptance_rule_refuses():
    c = RC.clip("d-outside")
    r, _ = round0(c)
    assert abs(r[4] * 1000.0 - c.initial_ms) >= 0.9 * c.radius_ms                      # rs_sync.rs:178 refuses it
    inside = round0(RC.clip("d+7.3"))[0]
    assert abs(inside[4] * 1000.0) < 0.9 * c.radius_ms and r[5] > 1000.0 * inside[5]   # and its cost is nowhere near a found delay's


def test_the_search_without_the_true_readout_time_costs_more_and_lands_farther():
    """a clean clip of 12 ms readout searched as a global shutter (0.01 ms): the per-point times are what makes the scene static"""
    c = RC.clip("d+7.3")
    true_r, _ = round0(c)
    flat_r, _ = round0(c, readout_ms=0.01)
    print("true readout: delay %.4f ms cost %.6g; 0.01 ms: delay %.4f ms cost %.6g" % (true_r[4] * 1e3, true_r[5], flat_r[4] * 1e3, flat_r[5]))
    assert flat_r[5] > true_r[5] and abs(flat_r[4] * 1000.0 - c.delay_ms) > abs(true_r[4] * 1000.0 - c.delay_ms)


def test_the_conjugate_track_convention_fails():
    """of q and its conjugate the statement takes the one under which a planted static scene is static.  Under the other, round 0 does not pick the nearest
    candidate in every search (it may in one, by the chance of 1 in 21), every pick costs several times more, and no final delay is within a gyro sample period"""
    hits = []
    for name in ("d+7.3", "d-41", "large-translation"):
        c = RC.clip(name)
        r, nearest = round0(c, conj=True)
        print("%s conjugate: round 0 %.1f ms (nearest %.1f) cost %.4g, final %.4f ms" % (name, r[2] * 1e3, nearest * 1e3, r[3], r[4] * 1e3))
        hits.append(r[2] == nearest)
        assert r[3] > 3.0 * round0(c)[0][3] and abs(r[4] * 1000.0 - c.delay_ms) > 1000.0 / c.rate_hz, (name, r)
    assert not all(hits), hits


def test_the_jacobi_direction_is_numpys_eigenvector():
    """the eigenvector of the smallest eigenvalue of sum m m^T within 1e-9 rad of numpy.linalg.eigh on the same matrix (a camera that moves: the eigenvalue is apart)"""
    worst = 0.0
    for name in ("large-translation", "d+7.3", "outliers-large"):
        c = RC.clip(name)
        T, Q = RS.track_seconds(c.track[0]), c.track[1]
        for pair in c.ranges[0][:3]:
            pr = RS.prepare(c.cam, c.cfg, pair[:2], pair[2], pair[3])
            d = np.array([c.delay_ms / 1000.0, c.delay_ms / 1000.0 + 0.004])
            ra = RS.to_world(RS.quat_at(T, Q, pr[1][None, :] + d[:, None]), pr[0])
            rb = RS.to_world(RS.quat_at(T, Q, pr[3][None, :] + d[:, None]), pr[2])
            m = ((ra[1] * rb[2]) - (ra[2] * rb[1]), (ra[2] * rb[0]) - (ra[0] * rb[2]), (ra[0] * rb[1]) - (ra[1] * rb[0]))
            M6 = RS.moments(m)
            t = RS.smallest(M6, c.cfg.sweeps)
            for k in range(2):
                A = np.array([[M6[0][k], M6[1][k], M6[2][k]], [M6[1][k], M6[3][k], M6[4][k]], [M6[2][k], M6[4][k], M6[5][k]]])
                w, V = np.linalg.eigh(A)
                assert w[1] - w[0] > 1e-3 * w[2]                                      # apart: the direction is defined
                v = V[:, 0]
                angle = np.arctan2(np.linalg.norm(np.cross(t[k], v)), abs(np.dot(t[k], v)))
                worst = max(worst, angle)
    print("worst angle to numpy's eigenvector: %.3g rad" % worst)
    assert worst < 1e-9


def test_the_statement_asserts_its_inputs_while_it_runs():
    c = RC.clip("d+7.3")
    T, Q = RS.track_seconds(c.track[0]), c.track[1]
    with pytest.raises(AssertionError):
        RS.quat_at(T[:1], Q[:1], np.array([1.0]))                                     # a track under 2 samples
    with pytest.raises(AssertionError):
        RS.quat_at(T, np.zeros_like(Q), np.array([1.0]))                              # a square root of 0
    bad = [(c.ranges[0][0][0], c.ranges[0][0][1], np.full((3, 2), np.nan, dtype=np.float32), np.zeros((3, 2), dtype=np.float32))]
    with pytest.raises(AssertionError):
        RS.search(c.cam, c.cfg, c.track[0], c.track[1], [bad], 0.0, 0.006)            # a result that is not finite


def test_the_edge_cases_of_a_pair():
    """a pair of 0 points costs 0; a pair of 1 point has hypothesis 0 only (its cost does not depend on the hypotheses' count); a range is its pairs' sum in order"""
    c = RC.case("emu-pinhole")
    T, Q = RS.track_seconds(c.track[0]), c.track[1]
    one = RS.prepare(c.cam, c.cfg, c.ranges[1][1][:2], c.ranges[1][1][2], c.ranges[1][1][3])
    assert len(one[1]) == 1
    d = np.array([0.0, 0.002])
    assert (RS.pair_costs(c.cfg, T, Q, one, d) == RS.pair_costs(RS.Cfg(readout_ms=12.0, hypotheses=0), T, Q, one, d)).all()
    none = tuple(x[:0] for x in one)
    assert (RS.pair_costs(c.cfg, T, Q, none, d) == 0.0).all()
    prepared = [RS.prepare(c.cam, c.cfg, p[:2], p[2], p[3]) for p in c.ranges[0]]
    per, total = RS.range_costs(c.cfg, T, Q, prepared, d)
    assert (total == (per[:, 0] + per[:, 1]) + per[:, 2]).all() and RS.round0_count(c.radius_s, c.cfg.step_s) == 5
