"""tests/_posestmt.py — the f32 statement gfw_pose_almeida is held to — held to its purpose: it recovers a planted rotation.

The reference's own output is not reproducible (its draws come from an unseeded generator) and nalgebra's source is not in the reference tree, so nothing
reference-produced can be compared; what the statement is FOR can.  Flows are planted by an independent float64 path (tests/_posecase.plant_f64: the f64 ray of `a`
rotated, projected, rounded to f32 pixels) on a pinhole camera, 0.5 .. 4.5 degrees about every axis, 0 .. 40 % of the points with gross outlier flows of 0.01 .. 0.05
in normalised units — at least 10 x the inlier gate (0.05 degrees read as 8.7e-4 normalised units, as the reference reads it), so the reference's logic alone has to
separate them.  The best round's inliers must be exactly the clean points, and the rotation must be within the angle 0.05 px subtend at the focal length,
0.05 / fx rad — about 400 f32 ULPs of a pixel coordinate, 30 x tighter than the gate."""
import numpy as np
import pytest

import _posecase as PC
import _posestmt as PS

# (points, rounds, (roll, pitch, yaw) degrees, outlier fraction, seed)
PLANTS = [(12, 32, (0.5, -1.0, 2.0), 0.0, 1), (40, 48, (-4.5, 0.5, 1.5), 0.25, 2), (150, 64, (2.5, 4.5, -0.5), 0.4, 3), (80, 200, (-1.5, -3.0, -4.5), 0.4, 4),
          (25, 64, (4.5, 4.5, 4.5), 0.2, 5)]


def rotation_error(Ra, Rb):
    c = (np.trace(np.asarray(Ra, dtype=np.float64).T @ np.asarray(Rb, dtype=np.float64)) - 1.0) / 2.0
    d = np.asarray(Ra, dtype=np.float64) - np.asarray(Rb, dtype=np.float64)
    return float(2.0 * np.arcsin(min(1.0, np.linalg.norm(d) / (2.0 * np.sqrt(2.0))))) if c > 0.9 else float(np.arccos(np.clip(c, -1.0, 1.0)))


@pytest.fixture(scope="module")
def recovered():
    out = []
    for n, rounds, angles, frac, seed in PLANTS:
        cam = PS.Camera(PC.pinhole_clip(), (960, 540), num_iters=rounds)
        a, b, R, clean = PC.plant_f64(cam, n, angles, frac, seed)
        triples, _ = PC.draws([n], rounds, cam.num_samples, 100 + seed, False)
        out.append((cam, R, clean, PS.estimate_pair(cam, a, b, triples[0])))
    return out


def test_the_best_rounds_inliers_are_exactly_the_clean_points(recovered):
    for (n, rounds, _, frac, _), (cam, R, clean, r) in zip(PLANTS, recovered):
        assert sorted(r["inlier_idx"].tolist()) == np.flatnonzero(clean).tolist(), (n, rounds, frac)
        assert r["best"][0] == int(clean.sum())


def test_the_planted_rotation_is_recovered_within_a_twentieth_of_a_pixel(recovered):
    worst = 0.0
    for (n, rounds, angles, frac, _), (cam, R, clean, r) in zip(PLANTS, recovered):
        err = rotation_error(R, r["rotation"])
        bar = 0.05 / cam.K[0, 0]
        print("planted %s deg, %d points, %d rounds, %.0f %% outliers: error %.3e deg (bar %.3e deg)" % (angles, n, rounds, 100 * frac, np.degrees(err), np.degrees(bar)))
        worst = max(worst, err / bar)
        assert err <= bar, (angles, n, rounds, np.degrees(err), np.degrees(bar))
    print("worst case: %.3e of the bar" % worst)


def test_an_all_outlier_pair_gives_the_identity():
    cam = PS.Camera(PC.pinhole_clip(), (960, 540), num_iters=16)
    a, b, _, clean = PC.plant_f64(cam, 30, (1.0, 1.0, 1.0), 1.0, 9)
    assert not clean.any()
    triples, _ = PC.draws([30], 16, cam.num_samples, 9, False)
    r = PS.estimate_pair(cam, a, b, triples[0])
    assert r["best"][0] < 3
    assert r["quat"].tolist() == [1.0, 0.0, 0.0, 0.0] and np.array_equal(r["rotation"], np.eye(3))


def test_two_rounds_with_the_same_triple_tie_and_the_earlier_wins():
    cam = PS.Camera(PC.pinhole_clip(), (960, 540), num_iters=3)
    a, b, _, clean = PC.plant_f64(cam, 20, (1.0, -2.0, 0.5), 0.2, 11)
    good = np.flatnonzero(clean)[:3]
    bad = np.flatnonzero(~clean)[:3]
    triples = np.array([bad, good, good], dtype=np.int32)
    r = PS.estimate_pair(cam, a, b, triples)
    assert r["round_inliers"][1] == r["round_inliers"][2] == int(clean.sum()) > r["round_inliers"][0]
    assert np.array_equal(r["round_fits"][1], r["round_fits"][2])
    assert r["best"] == (int(clean.sum()), 1)


def test_a_point_without_a_lens_inverse_rides_along_as_the_none_point():
    """tests/_posecase.none_case: opencv_standard with k1 = -0.12 has no inverse where 1 + k1 r^2 < 0 — point 5 lies that far outside the frame.  Its delta is
    (-1e6, -1e6) / size - pos for every rotation, so its derivative vectors are that too and it is never an inlier; the other points still give the planted rotation."""
    cam, a, b, q = PC.none_case()
    P = PS.prepare(cam, a, b)
    assert P["ray"][5, 2] == 0.0 and P["ray"][:5, 2].all() and P["ray"][6:, 2].all()
    want = np.array([PS.NONE_PT / np.float32(cam.video[0]) - P["pos"][5, 0], PS.NONE_PT / np.float32(cam.video[1]) - P["pos"][5, 1]], dtype=np.float32)
    assert all(np.array_equal(P["v"][5, k], want) for k in range(3))
    triples = np.array([[0, 1, 2], [5, 1, 2], [3, 4, 6]], dtype=np.int32)
    cam.num_iters = 3
    r = PS.estimate_pair(cam, a, b, triples)
    assert 5 not in r["inlier_idx"].tolist() and r["best"][0] == 11
    assert np.abs(r["quat"] - q).max() < 1e-5
