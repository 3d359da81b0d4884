"""gfw_pose_essential's kernels (gyroflow_amd/csrc/gfw_pose_essential.hip) interpreted on the host (tests/_emu_pose_essential.py) against the f64 statement
(tests/_posessstmt.py): quaternions, rotations, essential matrices, best rounds, every round's inliers and fit, bit for bit (a NaN is a NaN), over
tests/_posesscase.SPECS — pairs of 0, 7, 8, 9, 63, 64, 65 and 200 points, 1, 7, 64, 65 and 257 rounds (one more than a fit workgroup's lanes), a flow image of half
the video's size, the fisheye and the sony polynomial under a digital lens, a point without a lens inverse.  The statement's result of a case is computed once and
shared with tests/test_gpu_pose_essential.py."""
import numpy as np
import pytest

import _emu_pose_essential as EP
import _pairbase as PB
import _posesscase as EC


def run(c, rounds=True, octets=None):
    cam = c.cam
    return EP.pose_essential(cam.kp, cam.clip.model, cam.clip.digital, EC.cfg_of(cam), c.pairs, c.octets if octets is None else octets, rounds)


@pytest.mark.parametrize("name", sorted(EC.SPECS))
def test_interpreted_kernels_equal_the_statement_to_the_bit(name):
    c = EC.case(name)
    EC.assert_equal_to_statement(run(c), c.statement, name)


def test_the_cases_are_not_degenerate():
    """rounds differ in their inliers, the refit runs and finds a rotation for the larger pairs; pairs under 8 points have none"""
    quats, rot, ess, best, ri, rf = EC.case("fisheye-r7").statement
    big = [i for i, n in enumerate(EC.SIZES) if n >= 63]
    assert all(best[i, 0] >= 8 and best[i, 3] == 1 and quats[i, 0] != 1.0 and ess[i].any() for i in big), best.tolist()
    assert any(len(set(ri[i].tolist())) > 1 for i in big)
    for i, n in enumerate(EC.SIZES):
        if n < 8:
            assert quats[i].tolist() == [1.0, 0.0, 0.0, 0.0] and best[i].tolist() == [0, 0, 0, 0] and not ess[i].any() and not rf[i].any()
            assert np.array_equal(rot[i], np.eye(3))
    for name in ("sony-stretch-r65", "cvstd-none-r7", "fisheye-half-r7", "fisheye-r65"):
        best = EC.case(name).statement[3]
        assert best[:, 3].any(), (name, best.tolist())
    assert (EC.case("cvstd-none-r7").statement[3][0, 3]) == 1                         # the pair with the point that has no lens inverse


def test_without_round_outputs_the_work_space_serves():
    c = EC.case("fisheye-r1")
    got = run(c, rounds=False)
    EC.assert_equal_to_statement(got[:4], c.statement[:4], "fisheye-r1 without round outputs")
    assert (got[4] == -7).all() and (got[5] == -7.0).all()


def test_the_entry_points_check_names_the_pair():
    c = EC.case("fisheye-r64")
    o = np.array(c.octets)
    o[1, 5, 3] = 65
    with pytest.raises(EP.Refused, match="pair 1: round 5 draws 65 outside its 65 points"):
        run(c, octets=o)
    o = np.array(c.octets)
    o[0, 2, 7] = o[0, 2, 1]
    with pytest.raises(EP.Refused, match="pair 0: round 2 draws a point twice"):
        run(c, octets=o)
    o = np.array(c.octets)
    o[1, 63, 0] = -1
    with pytest.raises(EP.Refused, match="pair 1: round 63"):
        run(c, octets=o)


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged as given and the points from the arrays' start (tests/_pairbase.py)"""
    c = PB.essential()
    _, _, ess, _, ri, rf = PB.assert_base_does_not_matter(lambda: run(c), "pose_essential")
    assert ri.shape == (2, 4) and rf.any() and ri.any()                                    # the fits and the counts ran
