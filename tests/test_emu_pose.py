"""gfw_pose_almeida's kernels (gyroflow_amd/csrc/gfw_pose.hip) interpreted on the host (tests/_emu_pose.py) against the f32 statement (tests/_posestmt.py):
quaternions, rotations, best rounds, every round's inliers and fit, bit for bit, over tests/_posecase.SPECS — pairs of 0, 1, 2, 3, 12, 63, 64, 65 and 200 points,
1, 7, 64 and 65 rounds, num_samples 40 against 65 points with explicit lists, the fisheye and the sony polynomial under a digital lens, a point without a lens inverse.
The statement's result of a case is computed once and shared with tests/test_gpu_pose.py."""
import numpy as np
import pytest

import _emu_pose as EP
import _pairbase as PB
import _posecase as PC


def run(c, rounds=True, triples=None, samples="case"):
    cam = c.cam
    return EP.pose_almeida(cam.kp, cam.clip.model, cam.clip.digital, PC.cfg_of(cam), c.pairs, c.triples if triples is None else triples,
                           c.samples if samples == "case" else samples, rounds)


@pytest.mark.parametrize("name", sorted(PC.SPECS))
def test_interpreted_kernels_equal_the_statement_to_the_bit(name):
    c = PC.case(name)
    PC.assert_equal_to_statement(run(c), c.statement, name)


def test_the_cases_are_not_degenerate():
    """rounds differ in their inliers, the best round has at least 3 and the refit runs (a rotation other than the identity) — except under the strongly distorting
    lens, where the reference's estimator finds nothing (tests/_posecase.py says why) and the result is the identity"""
    quats, _, best, ri, _ = PC.case("fisheye-r7").statement
    big = [i for i, n in enumerate(PC.SIZES) if n >= 12]
    assert all(best[i, 0] >= 3 and quats[i, 0] != 1.0 for i in big)
    assert any(len(set(ri[i].tolist())) > 1 for i in big)
    assert all(quats[i].tolist() == [1.0, 0.0, 0.0, 0.0] and best[i].tolist() == [0, 0] for i, n in enumerate(PC.SIZES) if n < 3)
    quats, _, best, _, _ = PC.case("sony-stretch-r65-lists").statement
    assert best[0, 0] >= 3 and quats[0, 0] != 1.0
    quats, _, best, _, _ = PC.case("cvstd-none-r7").statement
    assert best[0, 0] >= 3 and quats[0, 0] != 1.0


def test_without_round_outputs_the_work_space_serves():
    c = PC.case("fisheye-r1")
    got = run(c, rounds=False)
    PC.assert_equal_to_statement(got[:3], c.statement[:3], "fisheye-r1 without round outputs")
    assert (got[3] == -7).all() and (got[4] == -7.0).all()


def test_the_entry_points_check_names_the_pair():
    c = PC.case("fisheye-r64-lists")
    t = np.array(c.triples)
    t[1, 5] = (3, 65, 4)
    with pytest.raises(EP.Refused, match="pair 1: round 5"):
        run(c, triples=t)
    t = np.array(c.triples)
    t[0, 2] = (4, 7, 4)
    with pytest.raises(EP.Refused, match="pair 0: round 2 draws a point twice"):
        run(c, triples=t)
    with pytest.raises(EP.Refused, match="pair 1: 65 points but num_samples 40"):
        run(c, samples=None)
    s = [np.array(x) for x in c.samples]
    s[1][63, 39] = 65
    with pytest.raises(EP.Refused, match="pair 1: sample 65 of round 63"):
        run(c, samples=s)


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged as given and the points from the arrays' start (tests/_pairbase.py)"""
    c = PB.almeida()
    quats, _, best, ri, _ = PB.assert_base_does_not_matter(lambda: run(c), "pose_almeida")
    assert best[1, 0] >= 3 and quats[1, 0] != 1.0 and ri.shape == (2, 4)                   # the fit, the count and the pick ran
