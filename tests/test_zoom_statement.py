"""The yardstick of the zoom search, checked on its own (CPU tier, no product code): the host statement of FovIterative::find_fov (tests/_zoomstmt.py) against
what the search is FOR.  A frame rendered by the oracle with fov = fov_minimal * 0.97 shows no background pixel, with fov_minimal * 1.03 at least one (at exactly
fov_minimal a sliver of under a pixel row can remain: the reference's search samples the outline; nothing here asserts on it).  Plus closed-form cases of find_fov
and of the smoothing's statement."""
import numpy as np
import pytest

import _zoomstmt as Z
import _zoomcase as ZC

CLIPS = {c.name: c for c in Z.statement_clips()}
FISHEYE = [n for n in CLIPS if n.startswith("fisheye-")]
LENSES = [n for n in CLIPS if n.endswith(("-r0-l1", "-r12-l0.6"))]
OTHERS = ["readout-neg", "readout-horizontal", "track-scale3", "digital-lens", "refraction", "margin2", "rotation90", "keyframed"]


def three_percent(clip, frames):
    fovs, _ = Z.clip_fovs(clip)
    for k in frames:
        f = fovs[k]
        inside, outside = ZC.background_pixels(clip, k, f * 0.97), ZC.background_pixels(clip, k, f * 1.03)
        print("%s frame %d: fov_minimal %.6f, background pixels %d at 0.97, %d at 1.03" % (clip.name, k, f, inside, outside))
        assert inside == 0, (clip.name, k, inside)
        assert outside >= 1, (clip.name, k, outside)


@pytest.mark.parametrize("name", FISHEYE)
def test_three_percent_property_fisheye(name):
    """320x180 source, outputs 320x180 and 240x180, readout 0 and 12 ms, lens correction 1.0 and 0.6, zoom centre (0, 0) and (0.04, -0.03): six frames each"""
    three_percent(CLIPS[name], (0, 4, 9, 13, 18, 23))


@pytest.mark.parametrize("name", LENSES)
def test_three_percent_property_every_physical_lens_model(name):
    """four frames x two settings on each of the nine physical lens models"""
    three_percent(CLIPS[name], (1, 8, 15, 22))


@pytest.mark.parametrize("name", OTHERS)
def test_three_percent_property_other_clips(name):
    three_percent(CLIPS[name], (2, 12) if name != "keyframed" else (2, 7, 12, 16, 23))


def test_identity_rotation_equal_aspects():
    """identity rotation, margin 0, output aspect = source aspect: every frame's fov is the same, and it is the extreme of the 120 mapped points"""
    clip = Z.Clip("identity", suppress=True)
    fovs, dbg = Z.clip_fovs(clip)
    assert np.all(fovs == fovs[0])
    w, h = clip.size
    poly = dbg[0] * np.array([w, h])
    ax, ay = np.abs(poly[:, 0] - w / 2.0), np.abs(poly[:, 1] - h / 2.0)
    a = h / w
    # the largest centred rectangle of aspect a inside the polygon: limited by the vertex whose max(|dx|, |dy| / a) is smallest
    extreme = float(np.min(np.maximum(ax, ay / a))) * 2.0 / w
    # equal, up to this f64 recomputation from the f32-normalised polygon (a few 1e-7 relative): the nearest vertex is a sampled one and the refinement accepts nothing
    assert abs(fovs[0] - extreme) <= 1e-6 * extreme, (fovs[0], extreme)
    trace = []
    Z.frame_fov(clip, 0, trace=trace)
    assert len(trace) == 1 and trace[0][2] is None, trace


def test_points_around_rect_order_and_count():
    rect = Z.points_around_rect(np.float32(320), np.float32(180), np.float32(2.0))
    assert len(rect) == Z.RECT_POINTS
    assert rect[0] == (2.0, 2.0) and rect[30] == (318.0, 2.0) and rect[60] == (318.0, 178.0) and rect[90] == (2.0, 178.0)
    assert len(Z.interpolate_points(rect[:3], 30)) == 63
    assert Z.USIZE_MAX % 120 == 15 and (2 ** 32 - 1) % 120 == 15                 # `idx.overflowing_sub(1).0 % len` at idx = 0


def test_smoothing_statement_on_a_series_with_one_dip():
    v = [1.0] * 40
    v[20] = 0.8
    fovs, mn = Z.zoom_smooth(v, -1.0, 30.0)
    assert fovs == [0.8] * 40 and mn == v                                         # static: the minimum everywhere
    for method in (0, 1):
        fovs, mn = Z.zoom_smooth(v, 0.5, 30.0, method)
        assert mn == v and all(a <= b + 1e-12 for a, b in zip(fovs, v)) and min(fovs) <= 0.8 + 1e-12 and (method == 1 or abs(fovs[0] - 1.0) < 1e-12)
    fovs, mn = Z.zoom_smooth(v, 0.0, 30.0)
    assert fovs == [1.0] * 40 and mn == v                                         # disabled
    v2 = [0.5 + 0.01 * i for i in range(40)]
    fovs, mn = Z.zoom_smooth(v2, -1.0, 30.0, 0, [(0.25, 0.5)])
    lo, hi = int(np.floor(39 * 0.25)), int(np.ceil(39 * 0.5))
    assert all(mn[i] == (v2[i] if lo <= i <= hi else max(v2)) for i in range(40))  # trim ranges: outside values become the maximum
    assert fovs == [v2[lo]] * 40
