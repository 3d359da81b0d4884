"""The zoom search's kernel SOURCE (gfw_zoom.hip), interpreted on the host (tests/_emu_zoom.py), against the host statement (tests/_zoomstmt.py) over the
statement clips: with caller-given rotations fov_minimal and the debug polygon are bit-identical; with rotations from the tracks they are held to the bar of
tests/test_gpu_zoom.py (twice the recorded sensitivity; on the host both sides call the same libm, so they agree to the bit here as well).

Rounds 2 to 4 of the refinement.  The loop is restated as written (gfw_zoom_rounds), and a test-only entry of the driver runs its fold and round logic over
tabulated polygons.  A polygon that makes round 2 REFINE does not exist, in any aspect: round 2's first fold walks the polygon that round 1's second fold has
just walked, from the state that fold ended in, and the state of nearest_edge never grows in either member under correctly rounded f32 arithmetic —
  * pred(fl(x)) <= x for every x > 0 (fl(x) is the float nearest to x), and rounding is monotone;
  * accepting (ap0, ap1) through `ap.1 > ap.0 * a` gives (fl(ap1 / a), ap1): ap1 < m1; and fl(ap1 / a) <= m0, because either m0 = fl(m1 / a), or
    m1 = fl(m0 * a) and then ap1 <= pred(m1) <= m0 * a, so ap1 / a <= m0;
  * accepting through the other branch gives (ap0, fl(ap0 * a)): ap0 < m0; and fl(ap0 * a) <= m1, because either m1 = fl(m0 * a), or m0 = fl(m1 / a) and
    then ap0 <= pred(m0) <= m1 / a, so ap0 * a <= m1 (the initial state is of the first kind) —
so a point rejected once stays rejected, and an accepted point is not strictly inside the state it produced.  test_a_second_walk_accepts_nothing searches for a
counter-example all the same (2 * 10^5 polygons clustered within ulps of a common edge, five aspects), and test_round_logic_over_tabulated_polygons drives the interpreted kernel's loop and the statement's through the exits that do exist."""
import json
import os

import numpy as np
import pytest

import _zoomstmt as Z
import _zoomcase as ZC
import _emu_zoom as E

CLIPS = {c.name: c for c in Z.statement_clips()}
SENS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoom_rotation_sensitivity.json")))["clips"]
f32 = np.float32


def same_f64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_given_rotations_bit_identical(name):
    clip = ZC.readout0(CLIPS[name])
    kp, search, frames, rot = ZC.inputs(clip, True)
    fov, dbg = E.zoom_fovs(kp, clip.model, clip.digital, search, frames, rotations=rot)
    ref_f, ref_d = Z.clip_fovs(clip, given_rotations=True)
    assert same_f64(fov, ref_f), (name, fov, ref_f)
    assert same_f64(dbg, ref_d), name


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_rotations_from_tracks(name):
    clip = CLIPS[name]
    kp, search, frames, _ = ZC.inputs(clip, False)
    fov, dbg = E.zoom_fovs(kp, clip.model, clip.digital, search, frames, tracks=clip.tracks, offsets=clip.sync_offsets, duration_ms=clip.duration_ms)
    ref_f, ref_d = Z.clip_fovs(clip)
    assert float(np.max(np.abs(fov - ref_f) / ref_f)) <= 2.0 * SENS[name]["fov_max_rel"], name
    assert float(np.max(np.abs(dbg - ref_d))) <= 2.0 * SENS[name]["polygon_max_abs"], name


def tabulated(rng, w, h, a, tight):
    """an outline and four refined polygons around the centred rectangle of half-width `e`: most points outside it, a few inside by ulps .. percents"""
    cx, cy = w / 2.0, h / 2.0
    e = rng.uniform(20.0, 0.45 * w)

    def poly(n, shrink):
        sx, sy = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
        k = 2.0 ** rng.integers(-23 if tight else -8, -2, n) * rng.integers(-2, 8, n)
        dx, dy = e * shrink * (1.0 + k), e * a * shrink * (1.0 + rng.permutation(k))
        pts = np.stack([cx + sx * dx, cy + sy * dy], axis=1)
        pts[rng.random(n) < 0.1] = -1000000.0                                      # the lens inverse's None
        return pts.astype(np.float32)
    return poly(120, 1.0), np.stack([poly(63, s) for s in (1.0 - 1e-3 * rng.integers(0, 3), 0.99, 0.98, 0.97)])


def test_round_logic_over_tabulated_polygons():
    rng = np.random.default_rng(20260)
    exits = {"none": 0, "second-none": 0, "second-some": 0}
    for case in range(240):
        w, h, out = [(320, 180, (320, 180)), (320, 180, (240, 180)), (180, 320, (9, 16)), (640, 360, (2560, 1080))][case % 4]
        a = out[1] / out[0]
        outline, refined = tabulated(rng, w, h, a, tight=case % 3 != 0)
        if case % 20 == 19:
            outline[:] = 2000000.0                                                  # nothing inside the initial rectangle: the loop leaves at once
        trace = []
        ref, _ = Z.find_fov(lambda k, pts: [(f32(x), f32(y)) for x, y in (outline if k == 0 else refined[k - 1])], w, h, out, 0.0, (0.0, 0.0), trace)
        got = E.zoom_table(outline, refined, w, h, out)
        assert same_f64([got], [ref]), (case, got, ref, trace)
        assert len(trace) <= 1, trace                                               # (the proof in the module docstring)
        exits["none" if not trace else "second-none" if trace[0][2] is None else "second-some"] += 1
    assert all(v >= 10 for v in exits.values()), exits


def test_a_second_walk_accepts_nothing():
    def fold(px, py, m0, m1, a):
        idx = np.full(px.shape[0], -1)
        for i in range(px.shape[1]):
            ap0, ap1 = px[:, i], py[:, i]
            acc = (ap0 < m0) & (ap1 < m1)
            b1 = ap1 > (ap0 * a).astype(f32)
            n0, n1 = np.where(b1, (ap1 / a).astype(f32), ap0), np.where(b1, ap1, (ap0 * a).astype(f32))
            m0, m1, idx = np.where(acc, n0, m0), np.where(acc, n1, m1), np.where(acc, i, idx)
        return m0, m1, idx
    rng = np.random.default_rng(5)
    for a in (f32(9.0 / 16.0), f32(0.75), f32(f32(1080.0) / f32(2560.0)), f32(f32(1.0) / f32(2.35)), f32(16.0 / 9.0)):
        n, k = 40000, 63
        base = rng.uniform(1.0, 400.0, (n, 1)).astype(f32)
        scale = 2.0 ** rng.integers(-24, -3, (n, k))
        px = (base * (1.0 + scale * rng.integers(-3, 4, (n, k)))).astype(f32)
        py = ((base * a).astype(f32) * (1.0 + scale * rng.integers(-3, 4, (n, k)))).astype(f32)
        m0, m1, first = fold(px, py, np.full(n, f32(1000000.0)), np.full(n, f32(f32(1000000.0) * a)), a)
        assert (first >= 0).all()
        _, _, again = fold(px, py, m0, m1, a)
        assert int((again >= 0).sum()) == 0, float(a)
