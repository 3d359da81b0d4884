"""tests/_posessstmt.py — the f64 statement gfw_pose_essential is held to — held to its purpose: it recovers a planted camera motion.

The reference's methods 0 and 2 call solvers that are not in the reference tree and draw from unseeded generators, so nothing reference-produced can be compared;
what the statement is FOR can.  The plant (tests/_posesscase.plant_scene) is an independent float64 path: a 3-D scene seen by a pinhole of 1920 x 1080 at f = 1000
before and after a rotation of up to 2 degrees an axis and a translation of length |t|, pixels rounded to f32, 30 % of the second frame's points displaced by up to
+-40 px; 120 points, 100 rounds, seeds 0 .. 3.

Bounds (tests/README_pose_essential.md records the measured figures):
  |t| >= 0.2    0.1 degrees: set in advance, tenfold the 0.009 degrees a numpy prototype of the scheme reached over four seeds
  |t| < 0.2     the problem is ill-conditioned (E degenerates as t -> 0): three times the statement's own measured worst over the committed seeds — 0.0616 degrees
                at |t| = 0.02 (bound 0.185), 0.0104 degrees at |t| = 0 (bound 0.0312)
  independent   the winning rotation against numpy's linalg.svd null vector and SVD decomposition on the same inlier set under the same selection rule, which pins
                the Jacobi solves and not the plant: the worst measured difference over all |t| and seeds is 1.6992e-11 degrees (at |t| = 0.02: 3e-13 rad, about a
                thousand f64 ULPs of a matrix entry — the conditioning of a null vector whose neighbouring eigenvalue is close); the bound is three times that,
                5.1e-11 degrees.  The front counts of both solutions must be equal at |t| >= 0.2"""
import numpy as np
import pytest

import _posecase as PC
import _posesscase as EC
import _posessstmt as ES
import _posestmt as PS

TS = (0.0, 0.02, 0.2, 0.5)
SEEDS = (0, 1, 2, 3)
BOUND_DEG = {0.0: 3 * 0.0104, 0.02: 3 * 0.0616, 0.2: 0.1, 0.5: 0.1}
INDEPENDENT_DEG = 3 * 1.6992e-11


def angle_deg(Ra, Rb):
    d = np.asarray(Ra, dtype=np.float64).reshape(3, 3) - np.asarray(Rb, dtype=np.float64).reshape(3, 3)
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(d) / (2.0 * np.sqrt(2.0))))))


def camera(rounds=100):
    return ES.Camera(EC.pinhole_clip(), (1920, 1080), num_iters=rounds)


@pytest.fixture(scope="module")
def recovered():
    out = {}
    for t in TS:
        for seed in SEEDS:
            cam = camera()
            a, b, R, clean = EC.plant_scene(cam, 120, t, seed)
            octets = EC.draws([120], 100, 100 + seed)
            out[t, seed] = (cam, a, b, R, clean, ES.estimate_pair(cam, a, b, octets[0]))
    return out


@pytest.mark.parametrize("t", TS)
def test_the_planted_rotation_is_recovered(recovered, t):
    worst = 0.0
    for seed in SEEDS:
        cam, a, b, R, clean, r = recovered[t, seed]
        err = angle_deg(R, r["rotation"])
        print("|t| = %g, seed %d: best %s of %d clean, error %.4e deg (bound %.4g)" % (t, seed, r["best"], int(clean.sum()), err, BOUND_DEG[t]))
        worst = max(worst, err)
        assert r["best"][3] == 1
    print("|t| = %g: worst %.4e deg" % (t, worst))
    assert worst <= BOUND_DEG[t]


def independent_rotation(x):
    """numpy's SVD null vector of the stacked kron rows and SVD decomposition of it, under the statement's selection rule (counts by least-squares depths)"""
    b1, b2 = ES.bearing(x[:, 0], x[:, 1]), ES.bearing(x[:, 2], x[:, 3])
    A = np.einsum("ni,nj->nij", b2, b1).reshape(-1, 9)
    E = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    x1, x2 = np.concatenate([x[:, :2], np.ones((len(x), 1))], axis=1), np.concatenate([x[:, 2:], np.ones((len(x), 1))], axis=1)
    best = None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        score = 0
        for t in (U[:, 2], -U[:, 2]):
            a = x1 @ R.T
            z = [np.linalg.lstsq(np.stack([a[i], -x2[i]], axis=1), -t, rcond=None)[0] for i in range(len(x))]
            score = max(score, sum(1 for z1, z2 in z if z1 > 0 and z2 > 0))
        if best is None or score > best[0] or (score == best[0] and np.trace(R) > best[1]):
            best = (score, np.trace(R), R)
    return best[2], best[0]


@pytest.mark.parametrize("t", TS)
def test_the_jacobi_solves_agree_with_numpys_svd_on_the_same_inliers(recovered, t):
    worst = 0.0
    for seed in SEEDS:
        cam, a, b, R, clean, r = recovered[t, seed]
        x = ES.prepare(cam, a, b).astype(np.float64)[r["inlier_idx"]]
        Ri, front = independent_rotation(x)
        diff = angle_deg(Ri, r["rotation"])
        print("|t| = %g, seed %d: statement against numpy %.4e deg, front %d / %d" % (t, seed, diff, r["best"][2], front))
        worst = max(worst, diff)
        if t >= 0.2:
            assert front == r["best"][2]
    print("|t| = %g: worst difference %.4e deg" % (t, worst))
    assert worst <= INDEPENDENT_DEG


def test_the_best_rounds_inliers_include_every_clean_point():
    for seed in SEEDS:
        cam = camera()
        a, b, R, clean = EC.plant_scene(cam, 120, 0.2, seed)
        r = ES.estimate_pair(cam, a, b, EC.draws([120], 100, 100 + seed)[0])
        assert set(np.flatnonzero(clean).tolist()) <= set(r["inlier_idx"].tolist()), seed
        assert r["best"][0] == len(r["inlier_idx"]) <= 120


def test_a_pure_rotation_picks_the_small_angle_candidate(recovered):
    """t = 0: E is degenerate and the two candidates' counts say little; the planted rotation is under 3.5 degrees, the twisted candidate turns by about 180"""
    for seed in SEEDS:
        r = recovered[0.0, seed][5]
        Ra, Rb, _ = ES.rotations_of(r["essential"])
        angles = sorted(angle_deg(np.eye(3), X) for X in (Ra, Rb))
        assert angles[0] < 4.0 and angles[1] > 170.0, angles
        assert angle_deg(np.eye(3), r["rotation"]) == angles[0]


def test_an_all_outlier_pair_has_no_rotation():
    cam = camera(16)
    a, b, _, clean = EC.plant_scene(cam, 30, 0.2, 9, outliers=1.0)
    assert not clean.any()
    r = ES.estimate_pair(cam, a, b, EC.draws([30], 16, 9)[0])
    assert r["best"][3] == 0 and r["best"][0] < 30
    assert r["quat"].tolist() == [1.0, 0.0, 0.0, 0.0] and np.array_equal(r["rotation"], np.eye(3))


def test_two_rounds_with_the_same_octet_tie_and_the_earlier_wins():
    cam = camera(3)
    a, b, _, clean = EC.plant_scene(cam, 40, 0.2, 11)
    good, bad = np.flatnonzero(clean)[:8], np.concatenate([np.flatnonzero(~clean)[:4], np.flatnonzero(clean)[8:12]])
    r = ES.estimate_pair(cam, a, b, np.array([bad, good, good], dtype=np.int32))
    assert r["round_inliers"][1] == r["round_inliers"][2] >= int(clean.sum()) > r["round_inliers"][0]
    assert np.array_equal(r["round_fits"][1], r["round_fits"][2])
    assert r["best"][:2] == (int(r["round_inliers"][1]), 1)


def test_a_point_without_a_lens_inverse_rides_along_as_the_none_point():
    """the first pair of the case "cvstd-none-r7": point 5 lies where opencv_standard with k1 < 0 has no inverse; it becomes (-1e6, -1e6) in both frames
    (cpu_undistort.rs:855) and takes part like any other point: rounds that draw it are fitted, it is scored by the same rule — a point that does not move is on
    its own epipolar line under any nearly skew E, so it may well count — and the pair still has a rotation"""
    c = EC.case("cvstd-none-r7")
    a, b = c.pairs[0]
    x = ES.prepare(c.cam, a, b)
    assert x[5].tolist() == [-1e6] * 4 and (np.abs(np.delete(x, 5, axis=0)) < 1.0).all()
    r = ES.estimate_pair(c.cam, a, b, c.octets[0])
    drawn = (c.octets[0] == 5).any(axis=1)
    assert drawn.any() and not drawn.all() and np.isfinite(r["round_fits"]).all() and r["round_fits"][drawn].any(axis=1).all()
    d = ES.sampson(r["round_fits"][r["best"][1]][None], x.astype(np.float64)[None])[0]
    assert np.isfinite(d[5]) and bool(d[5] <= c.cam.inlier_threshold) == (5 in r["inlier_idx"].tolist())
    assert r["best"][0] >= 8 and r["best"][3] == 1 and np.isfinite(r["rotation"]).all() and abs(np.linalg.det(r["rotation"]) - 1.0) < 1e-12


def test_record_almeida_on_the_moving_camera(recovered):
    """A record, not an assertion: the rotation-only Almeida statement on the |t| = 0.5 pairs beside this one's"""
    for seed in SEEDS:
        cam, a, b, R, clean, r = recovered[0.5, seed]
        acam = PS.Camera(EC.pinhole_clip(), (1920, 1080), num_iters=100)
        triples, _ = PC.draws([120], 100, acam.num_samples, 100 + seed, False)
        ra = PS.estimate_pair(acam, a, b, triples[0])
        print("|t| = 0.5, seed %d: essential %.4e deg (%d inliers), Almeida %.4e deg (%d inliers)"
              % (seed, angle_deg(R, r["rotation"]), r["best"][0], angle_deg(R, ra["rotation"]), ra["best"][0]))
