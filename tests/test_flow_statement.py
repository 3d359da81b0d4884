"""tests/_flowstmt.py — the fixed-point statement gfw_flow_pyrlk is held to — held to its purpose: it tracks a planted motion.

OpenCV's source is not part of the reference tree and OpenCV is not a dependency, so nothing reference-produced can pin the tracker; what the statement is FOR can.
tests/_flowcase.py renders an analytic texture under planted camera rotations (float64, then u8), so every point's true destination is known without resampling.
Over the features that lie at least 16 px inside both frames and outside the flat rectangle the statement's error against the analytic destination must be at most
0.1 px, at least three quarters of them must come back with status 1, and the pose statement (tests/_posestmt.py) must recover the planted rotation from the kept
points to better than 0.05 degrees, the estimator's own inlier angle.  The 0.1 px is derived from that chain, not from the tracker: at the scene's focal length of
600 px the inlier angle subtends 600 tan(0.05 deg) = 0.5236 px, and a fifth of that is 0.1047 px.

Measured here (this tier prints them; profiles/flow_pyrlk.txt records them): worst error 0.078 px (odd-384x216, pair (0, 2)), every selected feature tracked
(25 .. 43 a pair), worst rotation error 0.015 degrees."""
import numpy as np
import pytest

import _flowcase as FC
import _flowstmt as FS
import _posecase as PC
import _posestmt as PS
from test_pose_statement import rotation_error

CAP_PX, TRACKED_SHARE, CAP_DEG = 0.1, 0.75, 0.05
NAMES = sorted(FC.SPECS)


def pair_slices(c):
    raw = 0
    for a, b in FC.PAIRS:
        n = len(c.features[a])
        yield a, b, slice(raw, raw + n)
        raw += n


def interior(c, a, b):
    """the features of frame a that lie >= 16 px inside both frames and outside the flat rectangle -> (mask, true destinations)"""
    f = c.features[a].astype(np.float64)
    ok = np.isfinite(f).all(axis=1)
    g = np.where(ok[:, None], f, 0.0)
    dest = c.destination(a, b, g)
    deep = lambda p: (p[:, 0] >= 16) & (p[:, 0] <= c.width - 1 - 16) & (p[:, 1] >= 16) & (p[:, 1] <= c.height - 1 - 16)
    return ok & deep(g) & deep(dest) & ~c.in_flat(a, g), dest


def test_the_focal_length_makes_the_cap_a_fifth_of_the_inlier_angle():
    assert CAP_PX <= FC.FOCAL * np.tan(np.radians(CAP_DEG)) / 5.0
    for name in NAMES:
        assert FC.case(name).cam.K[0, 0] == FC.FOCAL and FC.case(name).cam.K[1, 1] == FC.FOCAL


@pytest.mark.parametrize("name", NAMES)
def test_the_planted_motion_is_tracked_within_a_tenth_of_a_pixel(name):
    c = FC.case(name)
    s = c.statement
    worst, motion = 0.0, 0.0
    for a, b, sl in pair_slices(c):
        sel, dest = interior(c, a, b)
        nxt, st = s["next"][sl].astype(np.float64), s["status"][sl]
        tracked = sel & (st == 1)
        err = np.linalg.norm(nxt - dest, axis=1)
        print("%s pair (%d, %d): %d features selected, %d tracked, worst error %.4f px, motion up to %.2f px" %
              (name, a, b, sel.sum(), tracked.sum(), err[tracked].max(), np.linalg.norm(dest - c.features[a], axis=1)[sel].max()))
        assert sel.sum() >= 20
        assert tracked.sum() >= TRACKED_SHARE * sel.sum(), (name, a, b, int(tracked.sum()), int(sel.sum()))
        assert err[tracked].max() <= CAP_PX, (name, a, b, err[tracked].max())
        worst, motion = max(worst, err[tracked].max()), max(motion, np.linalg.norm(dest - c.features[a], axis=1)[sel].max())
    print("%s: worst error %.4f px of %.1f" % (name, worst, CAP_PX))
    assert motion >= 5.0                                     # the pyramid is needed: more than the window's convergence range at level 0 alone is not claimed, but half a window


@pytest.mark.parametrize("name", NAMES)
def test_the_planted_rotation_is_recovered_from_the_kept_points(name):
    c = FC.case(name)
    s = c.statement
    first = s["pair_first"]
    for p, (a, b) in enumerate(FC.PAIRS):
        pa, pb = s["points_a"][first[p]:first[p + 1]], s["points_b"][first[p]:first[p + 1]]
        assert len(pa) >= 10
        triples, _ = PC.draws([len(pa)], c.cam.num_iters, c.cam.num_samples, 40 + p, False)
        r = PS.estimate_pair(c.cam, pa, pb, triples[0])
        err = np.degrees(rotation_error(c.rotation(a, b), r["rotation"]))
        print("%s pair (%d, %d): %d kept points, %d inliers, rotation error %.5f deg of %.2f" % (name, a, b, len(pa), r["best"][0], err, CAP_DEG))
        assert err < CAP_DEG, (name, a, b, err)


@pytest.mark.parametrize("name", NAMES)
def test_the_exits(name):
    c = FC.case(name)
    s = c.statement
    top = len(FS.level_sizes(c.width, c.height)) - 1
    for a, b, sl in pair_slices(c):
        f = c.features[a]
        nxt, st, it = s["next"][sl], s["status"][sl], s["iters"][sl]
        finite = np.isfinite(f).all(axis=1)
        inside = FS.inside(f, c.width, c.height)
        # the non-finite guard and the features outside the frame: not tracked, next = the feature (to the bit), no level ran
        assert (~finite).sum() == 2 and (finite & ~inside).sum() == 3
        assert (st[~inside] == 0).all() and (it[~inside] == -1).all()
        assert np.array_equal(nxt[~inside].view(np.uint32), f[~inside].view(np.uint32))
        # the flat patch: the features deep inside the rectangle (four are placed there) leave by the minEig exit at level 0 (status 0, level 0 skipped)
        deep = np.zeros(len(f), dtype=bool)
        deep[finite] = c.in_flat(a, f[finite].astype(np.float64), margin=-18.0)
        assert deep.sum() >= 4 and (st[deep] == 0).all() and (it[deep, 0] == -1).all()
        # the level cut: levels above L are not built
        assert (it[:, top + 1:] == -1).all() and (it[inside & ~deep, top] >= 0).any()
        # points whose motion leaves the frame are among the features: beyond the border the tracker sees the level's mirror image, so such a point may come back
        # lost (status 0), outside (dropped by the filter) or inside at a wrong place (the pose stage's outlier) — what is held is that the filter is the reference's
        gone = ~FS.inside(c.destination(a, b, np.where(finite[:, None], f, 0.0).astype(np.float64)), c.width, c.height) & inside
        assert gone.any()
        print("%s pair (%d, %d): %d features leave the frame: status %s, next %s" % (name, a, b, gone.sum(), st[gone].tolist(), nxt[gone].tolist()))
        kept = (st == 1) & FS.inside(nxt, c.width, c.height)
        p = FC.PAIRS.index((a, b))
        assert s["pair_first"][p + 1] - s["pair_first"][p] == kept.sum()
        assert np.array_equal(s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]], f[kept]) and np.array_equal(s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]], nxt[kept])


def test_the_level_cut():
    assert FS.level_sizes(200, 168) == [(200, 168), (100, 84), (50, 42)]                       # level 3 would be 25 x 21
    assert FS.level_sizes(384, 216) == [(384, 216), (192, 108), (96, 54), (48, 27)]
    assert FS.level_sizes(24, 24) == [(24, 24)] and FS.level_sizes(47, 8192) == [(47, 8192), (24, 4096)] and FS.level_sizes(185, 185)[-1] == (24, 24)
    # the window's indices iv - 1 .. iv + 22 with -21 <= iv <= n - 1 reflect into the level at every n >= 24
    for n in (24, 25, 27, 48):
        idx = FS.reflect(np.arange(-22, n + 22), n)
        assert idx.min() >= 0 and idx.max() <= n - 1


def test_the_out_of_level_exit_is_taken_through_every_side_at_level_0_and_above():
    """tests/_flowcase.ExitCase: ramps displaced so far that the updates walk the guess out of the level.  Which exit a feature takes is read from the statement's
    trace, and the outputs are held to it: a level-0 exit gives status 0 with level 0 ENTERED (iters[0] >= 0: 0 when the guess came down already outside, more when
    level 0's own updates carried it out); an upper level that is left hands down a guess that is outside level 0 as well (2 (g + 10) - 10 of a g outside
    [-21, n_1) is outside [-21, n_0)), so level 0 is left at once — the continuation.  The interpreter and device tiers compare this case to the bit, so the
    branch that keeps the J gathers inside the level is taken there through all four sides."""
    c = FC.case("exits-96x64")
    s, traces = c.statement, c.traces()
    w, h = c.width, c.height
    sides0, sides1, after_updates, converged_above = set(), set(), 0, 0
    for sl, rows in zip(FC.raw_slices(c), traces):
        for k, how in enumerate(rows):
            st, it, (nx, ny) = s["status"][sl][k], s["iters"][sl][k], s["next"][sl][k]
            gx, gy = nx - 10.0, ny - 10.0                                   # the last guess (next = g + 10)
            side = "x-" if gx < -21 else "x+" if gx >= w else "y-" if gy < -21 else "y+" if gy >= h else None
            if how.get(0) == "left":
                assert st == 0 and it[0] >= 0 and side is not None, (k, how, st, it, nx, ny)
                sides0.add(side)
                after_updates += it[0] >= 1
                converged_above += how.get(1) in ("converged", "oscillated")
            else:
                assert side is None or st == 0
            if how.get(1) == "left":
                assert 1 <= it[1] <= 30 and how.get(0) == "left" and it[0] == 0, (k, how, it)
                sides1.add(side)
            assert "guard" not in how.values()
    print("level-0 exits through %s, after an upper-level exit through %s; %d after updates of level 0, %d below a converged level 1" %
          (sorted(sides0), sorted(sides1), after_updates, converged_above))
    assert sides0 == {"x-", "x+", "y-", "y+"} and sides1 == {"x-", "x+", "y-", "y+"}
    assert after_updates >= 4 and converged_above >= 2


def test_the_guard_before_the_cast_cannot_be_reached_from_a_tracked_feature():
    """Why no case takes the `g not finite or |g| >= 2^24` exit: it cannot be reached.  A feature that is tracked lies in [0, 8192).  An update is only made from a
    guess inside [-21, n) (else the level is left), and its length is bounded: along an eigenvector of the accepted system, |d| = |b_e| / lambda with
    |b_e| <= sqrt(sum (J - I)^2 2^-20) sqrt(lambda) (Cauchy-Schwarz) and lambda >= 882 * 1e-4 (the minEig test), so |d| <= sqrt(441 * 8160^2 * 2^-20 / 0.0882) = 564 px,
    twice that for both components and f32 slack.  A guess therefore never exceeds n + 21 + 1200 at its level, at most 8 times that and 70 more three levels
    down: under 2^17.  The guard is there for the cast's sake (the issue's rule: a cast outside the int range is never executed, proven or not) and is stated, not
    exercised; what IS exercised is the out-of-level exit in front of the same cast (the test above)."""
    step = np.sqrt(441 * 8160.0 ** 2 * 2.0 ** -20 / (882 * 1e-4))
    assert 560 < step < 570 and (8192 + 21 + 2 * 600) * 8 + 70 < 2 ** 17 < 2 ** 24
    for name in sorted(FC.ALL_SPECS):                                      # the largest move any case's track makes is far inside that bound
        c = FC.case(name)
        s = c.statement
        feats = np.concatenate([c.features[a] for a, _ in c.pairs])
        ok = FS.inside(feats, c.width, c.height)
        assert np.abs(s["next"][ok] - feats[ok]).max() < (c.width + 21 + 1200)


def dis_grid_transcription(img):
    """opencv_dis.rs:62-119 line by line (the loop that chooses the points; the flow value itself is not part of it)"""
    h, w = img.shape
    step = w // 15
    window_size = max(int(np.floor(np.float64(np.float32(w) * np.float32(0.02)) + 0.5)), 10)
    half_win = window_size // 2
    points = []
    for i in range(0, w, step):
        for j in range(0, h, step):
            total, total_sq, count = np.float32(0.0), np.float32(0.0), np.float32(0.0)
            for ny in range(max(j - half_win, 0), min(j + half_win, h - 1) + 1):
                for nx in range(max(i - half_win, 0), min(i + half_win, w - 1) + 1):
                    pixel = np.float32(img[ny, nx])
                    total += pixel
                    total_sq += pixel * pixel
                    count += np.float32(1.0)
            mean = total / count
            if (total_sq / count) - (mean * mean) > np.float32(3.0):
                points.append((np.float32(i), np.float32(j)))
    return np.array(points, dtype=np.float32).reshape(-1, 2)


def test_the_grid_points_equal_the_transcription_on_a_frame_with_a_textureless_half():
    c = FC.case("cut-200x168")
    img = c.frames[0, :, :c.width].copy()
    img[:, c.width // 2:] = 77                                                                # the right half has no texture
    want = dis_grid_transcription(img)
    got = FS.grid_points(img)
    assert np.array_equal(got, want) and 20 < len(want) < 120 and (want[:, 0] <= c.width // 2 + 5).all()
    s = c.grid_statement
    for t in range(3):
        assert np.array_equal(s["grid_points"][t, :s["grid_counts"][t]], dis_grid_transcription(c.frames[t, :, :c.width]))
