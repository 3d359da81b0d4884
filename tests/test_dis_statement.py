"""The statement gfw_flow_dis is held to (tests/_disstmt.py) does what it is for, before anything is compared with it.

tests/_flowcase.py renders an analytic texture under planted camera rotations (float64, then u8), so every point's true destination is known without resampling.
The nodes that count are the "interior" ones: kept by the grid, at least 16 px inside both frames (the node and its analytic destination), and outside the flat
rectangle grown by 16 px, half a level-2 patch; at least 20 a pair.  The bars come from the pose stage, not from the flow: at the scenes' focal length of 600 px the
estimator's inlier angle of 0.05 degrees subtends 0.5236 px.  At the reference's finest scale 2 every interior node must lie within 0.5236 px of its analytic
destination (it is still an inlier of the true rotation) and tests/_posestmt.estimate_pair must recover the planted rotation from the returned points within 0.1
degrees; at the finest scale 1 the bars halve with the flow's pixel: 0.2618 px and 0.05 degrees, the project's own bar.

What the statement gives (printed by the tests; a float64 prototype of the scheme gave 0.375 px / 0.008 .. 0.048 degrees and 0.136 px / 0.003 .. 0.012 degrees):
  finest scale 2: 71 .. 82 interior nodes a pair, worst node 0.3755 px, rotation errors 0.007 .. 0.052 degrees
  finest scale 1: worst node 0.1226 px, rotation errors 0.002 .. 0.013 degrees
Every grid node comes back.  PyrLK on the same nodes: 0.0003 .. 0.007 degrees.  No variational refinement is part of the statement."""
import math

import numpy as np
import pytest

import _discase as DC
import _disstmt as DS
import _flowstmt as FS
import _posecase as PC
import _posestmt as PS
from test_pose_statement import rotation_error

INLIER_PX = 600.0 * math.tan(math.radians(0.05))
BARS = {2: (INLIER_PX, 0.1), 1: (INLIER_PX / 2.0, 0.05)}             # finest scale -> (px, degrees)
NAMES = sorted(DC.SPECS)


def test_the_bars_are_the_inlier_angle_at_the_scenes_focal_length():
    assert abs(INLIER_PX - 0.5236) < 5e-5 and abs(BARS[1][0] - 0.2618) < 5e-5
    for name in NAMES:
        assert DC.case(name).cam.K[0, 0] == 600.0 and DC.case(name).cam.K[1, 1] == 600.0


def interior(c, a, b, nodes):
    p = nodes.astype(np.float64)
    dest = c.destination(a, b, p)
    deep = lambda q: (q[:, 0] >= 16) & (q[:, 0] <= c.width - 1 - 16) & (q[:, 1] >= 16) & (q[:, 1] <= c.height - 1 - 16)
    return deep(p) & deep(dest) & ~c.in_flat(a, p, 16.0), dest


@pytest.mark.parametrize("finest", DC.FINEST)
@pytest.mark.parametrize("name", NAMES)
def test_every_interior_node_stays_an_inlier_and_the_planted_rotation_is_recovered(name, finest):
    c = DC.case(name)
    s, _ = DC.statement(name, finest)
    cap_px, cap_deg = BARS[finest]
    first, motion = s["pair_first"], 0.0
    for p, (a, b) in enumerate(c.pairs):
        pa, pb = s["points_a"][first[p]:first[p + 1]], s["points_b"][first[p]:first[p + 1]]
        # every node the grid keeps is returned, in grid order
        assert np.array_equal(pa, FS.grid_points(c.frames[a, :, :c.width])) and len(pa) == s["grid_counts"][a] and len(pb) == len(pa)
        sel, dest = interior(c, a, b, pa)
        err = np.linalg.norm(pb.astype(np.float64) - dest, axis=1)
        triples, _ = PC.draws([len(pa)], c.cam.num_iters, c.cam.num_samples, 40 + p, False)
        r = PS.estimate_pair(c.cam, pa, pb, triples[0])
        deg = np.degrees(rotation_error(c.rotation(a, b), r["rotation"]))
        far = np.linalg.norm(dest - pa, axis=1)[sel].max()
        print("%s finest %d pair (%d, %d): %d nodes, %d interior, worst node %.4f px of %.4f, rotation error %.5f deg of %.2f, motion up to %.2f px" %
              (name, finest, a, b, len(pa), sel.sum(), err[sel].max(), cap_px, deg, cap_deg, far))
        assert sel.sum() >= 20
        assert err[sel].max() <= cap_px, (name, finest, a, b, err[sel].max())
        assert deg <= cap_deg, (name, finest, a, b, deg)
        if (a, b) == (0, 2):
            motion = far
    assert motion > 5.0                                      # pair (0, 2): the pyramid is needed


def test_the_displaced_ramps_take_the_return_to_the_start_value():
    """exits-96x64: ramps displaced by +-40 and 12 px.  The trace names the patches that end a pass more than 8 level pixels from their start value and return to it;
    the clamped sampling is taken through every side (the statement asserts every index it forms)."""
    for finest in DC.FINEST:
        s, traces = DC.statement("exits-96x64", finest)
        back = [t for tr in traces for t in tr]
        print("exits-96x64 finest %d: returns to the start value (level, pass, patch) per pair: %s" % (finest, [tr for tr in traces]))
        assert len(back) >= 1 and all(l >= finest for l, _, _ in back)
        assert np.isfinite(s["points_b"]).all() and np.isfinite(s["flow"]).all()
    # the analytic scenes take no return: their motion stays within the rule at every level
    assert not any(t for tr in DC.statement("cut-200x168", 2)[1] for t in tr)
    # sampling far outside on every side lands on the replicated edge, and forms no index outside the level
    B = np.arange(24 * 16, dtype=np.uint8).reshape(16, 24)
    x, y = np.array([0, 23, 5, 5]), np.array([3, 3, 0, 15])
    ux, uy = np.array([-1e9, 1e9, 0.0, 0.0], dtype=np.float32), np.array([0.0, 0.0, -40.5, 40.5], dtype=np.float32)
    assert DS.sample(B, x, y, ux, uy).tolist() == [32 * int(B[3, 0]), 32 * int(B[3, 23]), 32 * int(B[0, 5]), 32 * int(B[15, 5])]


def test_the_level_sizes_and_the_coarsest_scale():
    for size, levels in DC.LEVELS.items():
        assert DS.level_sizes(*size) == levels and DS.coarsest_scale(*size) == len(levels) - 1, size
    assert DS.coarsest_scale(*DC.REFUSED_SIZE) == 1                 # under the reference's finest scale: refused there, served at 1
    assert DS.coarsest_scale(1280, 720) == 5 and DS.coarsest_scale(8192, 8192) == 8
    with pytest.raises(AssertionError):
        DS.flow_dis(np.zeros((2, 24, 256), dtype=np.uint8), [(0, 1)], 2)
    # level 3 of 200 x 168 is 25 x 21: the halved odd side is not read, and the last row (20) lies under no patch: it takes row 19's value
    c = DC.case("cut-200x168")
    pyr = DS.pyramid(c.frames[0, :, :c.width])
    assert [p.shape for p in pyr] == [(168, 200), (84, 100), (42, 50), (21, 25)]
    assert np.array_equal(pyr[3], ((pyr[2][0:42:2, 0:50:2].astype(int) + pyr[2][0:42:2, 1:50:2] + pyr[2][1:42:2, 0:50:2] + pyr[2][1:42:2, 1:50:2] + 2) >> 2))
    L = DS.Level(pyr[3], DS.pyramid(c.frames[1, :, :c.width])[3])
    assert (L.nx, L.ny) == (5, 4)
    U = L.dense(np.random.default_rng(3).uniform(-1, 1, (20, 2)).astype(np.float32))
    assert np.array_equal(U[20], U[19]) and np.array_equal(U[:, 24], U[:, 23]) and not np.array_equal(U[19], U[18])
