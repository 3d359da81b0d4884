"""tests/_cornerstmt.py — the statement gfw_corners_shi_tomasi is held to — held to its purpose: it finds corners, and what it finds tracks.

OpenCV's source is not part of the reference tree and OpenCV is not a dependency, so nothing reference-produced can pin the detector; what the statement is FOR can.
On four rectangles over a flat background (clean, and with +-2 gray levels of noise) the corners must be EXACTLY the 16 rectangle-corner pixels: nothing on an
edge, nothing in the flat parts.  On the analytic scenes of tests/_flowcase.py no corner may lie in the flat rectangle; the accepted corners are pairwise at least
min_distance apart and come in descending key order; where the cap is not reached every candidate above the threshold that was not picked lies within reach of an
earlier pick.  The two equivalent forms the device uses (the local maximum on raw e; the arg-max rounds instead of a sorted walk) are shown equal to the stated
ones on every case and variant.  Then the chain: the detected corners go through tests/_flowstmt.flow_pyrlk and tests/_posestmt on both analytic scenes under the
bars of tests/test_flow_statement.py (0.1 px, three quarters tracked, 0.05 degrees).

Measured here (this tier prints them; profiles/corners.txt records them): every interior corner tracked (108 .. 151 a pair), worst error 0.060 px (cut-200x168,
pair (0, 2)), worst rotation error 0.0101 degrees."""
import numpy as np
import pytest

import _cornercase as CC
import _cornerstmt as CS
import _flowcase as FC
import _posecase as PC
import _posestmt as PS
from test_flow_statement import CAP_DEG, CAP_PX, TRACKED_SHARE
from test_pose_statement import rotation_error

SCENES = sorted(FC.SPECS)


def frames_of(name):
    c = CC.case(name)
    return [c.frames[f][:, :c.width] for f in range(len(c.frames))]


@pytest.mark.parametrize("name", ["rects-160x120", "rects-noise-160x120"])
def test_the_corners_of_rectangles_are_exactly_their_corner_pixels(name):
    stats = {}
    corners, scores = CS.detect(frames_of(name)[0], stats=stats)
    assert sorted((int(x), int(y)) for x, y in corners) == CC.rect_corner_pixels()                      # at distance 0, nothing on an edge
    assert (corners == np.rint(corners)).all() and (scores > stats["threshold"]).all() and (np.diff(scores) <= 0).all()


@pytest.mark.parametrize("name", SCENES)
def test_no_corner_lies_in_the_flat_rectangle(name):
    """e of a pixel reads the 5 x 5 pixels around it: 3 px inside the rectangle (2, and the rounding of the planted motion) every one of them is 128"""
    c, s = FC.case(name), CC.statement(name)
    for t in range(3):
        p = s["corners"][t, :s["counts"][t]].astype(np.float64)
        assert not c.in_flat(t, p, margin=-3.0).any()
        ys, xs = np.mgrid[0:c.height, 0:c.width]
        deep = c.in_flat(t, np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float64), margin=-3.0).reshape(c.height, c.width)
        assert deep.sum() > 2000 and (CS.min_eigen(frames_of(name)[t])[deep] == 0.0).all()


@pytest.mark.parametrize("variant", CC.VARIANTS, ids=CC.VARIANT_IDS)
@pytest.mark.parametrize("name", CC.NAMES)
def test_the_pick_keeps_its_distance_and_its_order_and_the_two_forms_agree(name, variant):
    c = CC.case(name)
    m, q, d = variant["max_corners"], variant["quality"], variant["min_distance"]
    s = CC.statement(name, **variant)
    for f, img in enumerate(frames_of(name)):
        e = CS.min_eigen(img)
        t = CS.threshold(e, q)
        cand = CS.candidates(e, t)
        assert np.array_equal(cand, CS.candidates_raw(e, t))                                           # the local maximum on raw e
        assert not cand[0].any() and not cand[-1].any() and not cand[:, 0].any() and not cand[:, -1].any()
        n = s["counts"][f]
        pts = s["corners"][f, :n].astype(np.int64)
        key = (s["scores"][f, :n].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (pts[:, 1] * c.width + pts[:, 0]).astype(np.uint64)
        assert (np.diff(key.astype(object)) < 0).all()                                                 # descending, unique
        assert cand[pts[:, 1], pts[:, 0]].all() and (s["corners"][f, n:] == 0).all() and (s["scores"][f, n:] == 0).all()
        if d >= 1 and n > 1:
            d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2).astype(np.float32)
            np.fill_diagonal(d2, np.inf)
            assert not (d2 < np.float32(d) * np.float32(d)).any()
        all_keys = CS.keys(e, cand)
        if n < m:                                                                                       # the list was exhausted: nothing above the threshold was left out without a reason
            left = np.setdiff1d(all_keys, key)
            assert n + len(left) == len(all_keys)
            for k in left:
                idx = int(k & np.uint64(0xFFFFFFFF))
                near = CS._near(idx % c.width, idx // c.width, pts[:, 0], pts[:, 1], d)
                assert d >= 1 and (near & (key > k)).any()
        # the arg-max rounds over every positive local maximum (the device's list) = the sorted walk over the candidates
        stats = {}
        rounds = CS.pick_rounds(CS.keys(e, CS.candidates_raw(e, np.float32(0.0))), c.width, m, d, t, stats)
        assert np.array_equal(rounds, key) and np.array_equal(CS.pick_rounds(all_keys, c.width, m, d), key)
        assert stats["rounds"] <= m and stats["rounds"] in (n, n + 1)


@pytest.mark.parametrize("name", CC.NAMES)
def test_every_box_sum_is_below_two_to_the_24(name):
    for img in frames_of(name):
        dx, dy = CS.derivatives(img)
        assert np.abs(dx).max() <= 1020 and np.abs(dy).max() <= 1020
        for s in CS.box_sums(img):
            assert np.abs(s).max() < 2 ** 24
    assert 9 * 1020 ** 2 < 2 ** 24


def test_the_product_maps_are_reflected_not_the_image():
    """The box filter reflects Dx Dy itself.  The Sobel of a reflected image would give the border row's outer neighbour the mirrored Dy = -Dy: Sxy differs there."""
    img = frames_of("noise-40x48")[0]
    dx, dy = CS.derivatives(img)
    sxy = CS.box_sums(img)[1]
    p = (dx * dy).astype(np.int64)
    assert sxy[0, 5] == 2 * p[1, 4:7].sum() + p[0, 4:7].sum()                                            # row -1 is row 1 of the product map
    pad = np.pad(img.astype(np.int32), 2, mode="reflect")                                               # .. not the product of the derivatives of a reflected image
    gx = lambda y, x: (pad[y - 1, x + 1] - pad[y - 1, x - 1]) + 2 * (pad[y, x + 1] - pad[y, x - 1]) + (pad[y + 1, x + 1] - pad[y + 1, x - 1])
    gy = lambda y, x: (pad[y + 1, x - 1] - pad[y - 1, x - 1]) + 2 * (pad[y + 1, x] - pad[y - 1, x]) + (pad[y + 1, x + 1] - pad[y - 1, x + 1])
    other = sum(gx(y + 2, x + 2) * gy(y + 2, x + 2) for y in (-1, 0, 1) for x in (4, 5, 6))
    assert other != sxy[0, 5]


def test_a_pure_edge_is_no_corner():
    img = np.zeros((8, 8), dtype=np.uint8)
    img[:, 4:] = 255                                                                                    # e is 0 or a rounding below it: the threshold is max(e, 0) * quality
    e = CS.min_eigen(img)
    assert e.max() <= 0.0 and len(CS.detect(img)[0]) == 0 and CS.threshold(e, 0.01) == 0.0


def interior(c, a, b, feats):
    """the corners of frame a that lie >= 16 px inside both frames and outside the flat rectangle -> (mask, true destinations)"""
    g = feats.astype(np.float64)
    dest = c.destination(a, b, g)
    deep = lambda p: (p[:, 0] >= 16) & (p[:, 0] <= c.width - 1 - 16) & (p[:, 1] >= 16) & (p[:, 1] <= c.height - 1 - 16)
    return deep(g) & deep(dest) & ~c.in_flat(a, g), dest


@pytest.mark.parametrize("name", SCENES)
def test_the_detected_corners_track_and_give_the_planted_rotation(name):
    c = FC.case(name)
    feats, s = CC.chain(name)
    raw, worst = 0, 0.0
    for p, (a, b) in enumerate(FC.PAIRS):
        n = len(feats[a])
        sl = slice(raw, raw + n)
        raw += n
        sel, dest = interior(c, a, b, feats[a])
        nxt, st = s["next"][sl].astype(np.float64), s["status"][sl]
        tracked = sel & (st == 1)
        err = np.linalg.norm(nxt - dest, axis=1)
        print("%s pair (%d, %d): %d corners, %d interior, %d of them tracked, worst error %.4f px" % (name, a, b, n, sel.sum(), tracked.sum(), err[tracked].max()))
        assert sel.sum() >= 20
        assert tracked.sum() >= TRACKED_SHARE * sel.sum(), (name, a, b, int(tracked.sum()), int(sel.sum()))
        assert err[tracked].max() <= CAP_PX, (name, a, b, err[tracked].max())
        worst = max(worst, err[tracked].max())
    print("%s: worst error %.4f px of %.1f" % (name, worst, CAP_PX))
    for p, ((a, b), (pa, pb)) in enumerate(zip(FC.PAIRS, CC.chain_pairs(name))):
        assert len(pa) >= 10
        triples, _ = PC.draws([len(pa)], c.cam.num_iters, c.cam.num_samples, 40 + p, False)
        r = PS.estimate_pair(c.cam, pa, pb, triples[0])
        err = np.degrees(rotation_error(c.rotation(a, b), r["rotation"]))
        print("%s pair (%d, %d): %d kept points, %d inliers, rotation error %.5f deg of %.2f" % (name, a, b, len(pa), r["best"][0], err, CAP_DEG))
        assert err < CAP_DEG, (name, a, b, err)
