"""The statement gfw_flow_dis_refined is held to (tests/_varrefstmt.py) does what refinement is for, before anything is compared with it.

The scenes, the interior-node rule and the bars are those of tests/test_dis_statement.py (imported): every interior node within 0.5236 px of its analytic
destination at the finest scale 2 and 0.2618 px at 1, the planted rotation recovered by tests/_posestmt.estimate_pair within 0.1 and 0.05 degrees.  On top of that,
in EVERY pair the mean interior node error is lower than that of the unrefined statement (tests/_discase.statement) and the worst one is not higher.  Both series
are printed.  What the statement gives (worst / mean interior node in px, unrefined -> refined, and the refined rotation error, per pair):
  cut-200x168 finest 2   0.2851 / 0.1300 -> 0.1983 / 0.0640, 0.2496 / 0.0990 -> 0.1795 / 0.0820, 0.2502 / 0.1168 -> 0.2278 / 0.0918; 0.055, 0.065, 0.066 deg
  cut-200x168 finest 1   0.1161 / 0.0479 -> 0.0572 / 0.0305, 0.1164 / 0.0444 -> 0.0521 / 0.0208, 0.1110 / 0.0387 -> 0.0719 / 0.0329; 0.031, 0.020, 0.029 deg
  odd-384x216 finest 2   0.2752 / 0.1220 -> 0.1786 / 0.0710, 0.2419 / 0.1142 -> 0.2036 / 0.0950, 0.3755 / 0.1429 -> 0.2815 / 0.1094; 0.018, 0.021, 0.034 deg
  odd-384x216 finest 1   0.1002 / 0.0389 -> 0.0546 / 0.0257, 0.1226 / 0.0409 -> 0.0558 / 0.0215, 0.1163 / 0.0448 -> 0.0792 / 0.0325; 0.009, 0.004, 0.009 deg"""
import numpy as np
import pytest

import _discase as DC
import _disstmt as DS
import _posecase as PC
import _posestmt as PS
import _varrefcase as VC
import _varrefstmt as VS
from test_dis_statement import BARS, NAMES, interior
from test_pose_statement import rotation_error


@pytest.mark.parametrize("finest", DC.FINEST)
@pytest.mark.parametrize("name", NAMES)
def test_refinement_lowers_every_pairs_node_error_within_the_bars(name, finest):
    c = DC.case(name)
    plain, _ = DC.statement(name, finest)
    s = VC.statement(name, finest)
    cap_px, cap_deg = BARS[finest]
    first = s["pair_first"]
    assert np.array_equal(first, plain["pair_first"]) and np.array_equal(s["points_a"], plain["points_a"]) and np.array_equal(s["grid_counts"], plain["grid_counts"])
    for p, (a, b) in enumerate(c.pairs):
        pa, pb, pb0 = s["points_a"][first[p]:first[p + 1]], s["points_b"][first[p]:first[p + 1]], plain["points_b"][first[p]:first[p + 1]]
        sel, dest = interior(c, a, b, pa)
        err = np.linalg.norm(pb.astype(np.float64) - dest, axis=1)[sel]
        err0 = np.linalg.norm(pb0.astype(np.float64) - dest, axis=1)[sel]
        triples, _ = PC.draws([len(pa)], c.cam.num_iters, c.cam.num_samples, 40 + p, False)
        deg = np.degrees(rotation_error(c.rotation(a, b), PS.estimate_pair(c.cam, pa, pb, triples[0])["rotation"]))
        print("%s finest %d pair (%d, %d): %d interior nodes, worst %.4f -> %.4f px of %.4f, mean %.4f -> %.4f px, rotation error %.5f deg of %.2f" %
              (name, finest, a, b, sel.sum(), err0.max(), err.max(), cap_px, err0.mean(), err.mean(), deg, cap_deg))
        assert sel.sum() >= 20
        assert err.max() <= cap_px, (name, finest, a, b, err.max())
        assert deg <= cap_deg, (name, finest, a, b, deg)
        assert err.mean() < err0.mean(), (name, finest, a, b, err0.mean(), err.mean())
        assert err.max() <= err0.max(), (name, finest, a, b, err0.max(), err.max())


@pytest.mark.parametrize("finest", DC.FINEST)
def test_the_displaced_ramps_stay_finite(finest):
    """exits-96x64: ramps displaced by +-40 and 12 px, so the warp clamps through every side (the statement asserts every index, square root, A11 / A22 and result
    while it runs).  Nothing is held to a position there."""
    s = VC.statement("exits-96x64", finest)
    assert np.isfinite(s["points_b"]).all() and np.isfinite(s["flow"]).all()
    assert not np.array_equal(s["flow"], DC.statement("exits-96x64", finest)[0]["flow"])


def test_no_fixed_point_iteration_is_the_unrefined_statement_to_the_bit():
    c = DC.case("cut-200x168")
    s = VS.flow_dis_refined(c.frames[:, :, :c.width], c.pairs, 2, VS.DEFAULT._replace(fixed_point_iters=0))
    DC.assert_equal_to_statement(s, DC.statement("cut-200x168", 2)[0], "fixed_point_iters = 0")


def test_a_constant_field_over_identical_frames_comes_back_to_the_bit():
    """Iz = 0 makes b1 = b2 = 0, the Laplacian of a constant is 0, so B1 = B2 = 0 and du = dv = 0 is the fixed point of every sweep.  The constant is a whole number of
    pixels and the frame periodic in it away from the edge; at the edge the replicated sample differs, so the frame is constant there: a constant frame pair."""
    A = np.full((16, 24), 93, dtype=np.uint8)
    for value in ((0.0, 0.0), (3.0, -2.0), (0.37, -1.61)):
        U = np.broadcast_to(np.array(value, dtype=np.float32), (16, 24, 2)).copy()
        R = VS.refine(A, A, U, VS.DEFAULT)
        assert R is not U and np.array_equal(R.view(np.uint32), U.view(np.uint32)), value
    # a textured frame against itself under the zero field
    T = DC.case("cut-200x168").frames[0, :64, :96]
    Z = np.zeros((64, 96, 2), dtype=np.float32)
    assert np.array_equal(VS.refine(T, T, Z, VS.DEFAULT), Z)


def test_the_two_colours_update_every_pixel_of_an_odd_width_level_exactly_once():
    g = np.random.default_rng(5)
    A, B = g.integers(0, 256, (8, 9)).astype(np.uint8), g.integers(0, 256, (8, 9)).astype(np.uint8)
    trace = []
    R = VS.refine(A, B, g.uniform(-1, 1, (8, 9, 2)).astype(np.float32), VS.Cfg(2, 3, 20.0, 5.0, 10.0, 1.6), trace)
    assert np.isfinite(R).all() and len(trace) == 2 * 3 * 2
    yy, xx = np.mgrid[0:8, 0:9]
    for k in range(0, len(trace), 2):
        (_, fp, it, c0, m0), (_, fp1, it1, c1, m1) = trace[k], trace[k + 1]
        assert (fp, it, c0, c1) == (fp1, it1, 0, 1) and (fp, it) == (k // 6, k // 2 % 3)
        assert (m0.astype(int) + m1.astype(int) == 1).all()                     # every pixel once
        assert np.array_equal(m0, (xx + yy) % 2 == 0) and m0.sum() == 36 and m1.sum() == 36
        # a colour's pixels have no neighbour of their own colour: the order within a colour is free
        assert not (m0[:, 1:] & m0[:, :-1]).any() and not (m0[1:] & m0[:-1]).any()


def test_the_configuration_changes_the_result():
    assert not np.array_equal(VC.statement("cut-200x168", 2, VC.OTHER)["flow"], VC.statement("cut-200x168", 2)["flow"])
