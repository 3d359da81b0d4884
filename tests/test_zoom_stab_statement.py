"""The yardstick of gfw_zoom_fovs_stab, checked on its own (CPU tier, no product code): the zoom search's host statement with per-point IBIS/OIS shifts
(tests/_zoomstab.py) against what the search is FOR, as tests/test_zoom_statement.py holds the plain statement.  Clips with IBIS/OIS splines, with and without
rolling shutter, are rendered by the oracle with the matching m[9..13] in their rows (_hoststmt.row_matrices_from_tracks): at 0.97 x fov_minimal no pixel of ANY
frame shows background, at 1.03 x every frame does.

The spline amplitudes (_zoomstab.IBIS_XY = 20, OIS_XY = 8, ROLL = 100 sensor units: about a pixel of displacement at 320 x 180 in all) are chosen for the
reference's semantics themselves: a frame without rolling shutter shifts ONE outline point in the search while the render shifts the whole frame, so the search is
blind to the shift and the 3 % band (4.8 px / 2.7 px) has to absorb it.  Meshes need no purpose test: their mapping is the oracle's."""
import numpy as np
import pytest

import _zoomstmt as Z
import _zoomstab as ZS

CLIPS = {c.name: c for c in ZS.stab_clips()}


@pytest.mark.parametrize("name", ZS.PURPOSE)
def test_three_percent_property_with_stabiliser_shifts_every_frame(name):
    clip = CLIPS[name]
    fovs, _ = ZS.clip_fovs(clip)
    plain, _ = Z.clip_fovs(clip)
    shifted = 0
    for k in range(len(clip.timestamps)):
        f = fovs[k]
        inside, outside = ZS.background_pixels(clip, k, f * 0.97), ZS.background_pixels(clip, k, f * 1.03)
        print("%s frame %d: fov_minimal %.6f (without the shifts %.6f), background pixels %d at 0.97, %d at 1.03" % (name, k, f, plain[k], inside, outside))
        assert inside == 0, (name, k, inside)
        assert outside >= 1, (name, k, outside)
        shifted += f != plain[k]
        if clip._stabs[k] is None:
            assert f == plain[k], (name, k)                                       # no camera_stab_data entry: the plain statement's frame
    if abs(clip.readout) > 0.0:
        assert shifted >= 4, (name, shifted)                                      # every point is shifted: the shifts do move the result (without rolling shutter only
                                                                                  # where point 0 of a mapped set decides: tests/test_emu_zoom_stab.py has that case)


def test_the_rows_of_the_render_carry_the_shift_terms():
    clip = CLIPS["shifts-r12"]
    t = ZS.stab_terms(clip, 0, 180)
    assert t.shape == (180, 5) and 0.05 < np.abs(t[:, :2]).max() < 0.7 and np.abs(t[:, 2]).max() < 0.1 * np.pi / 180.0 * 1.001 and np.ptp(t[:, 0]) > 0.01
    assert ZS.stab_terms(clip, 2, 180) is None


def test_without_data_the_statement_is_the_plain_one():
    clip = ZS.StabClip("plain", stab=None, mesh=None, readout=12.0)
    a, ad = ZS.clip_fovs(clip, frames=range(4))
    b, bd = Z.clip_fovs(clip)
    assert np.array_equal(a, b[:4]) and np.array_equal(ad, bd[:4])


def test_one_shift_goes_to_index_zero_only():
    """no rolling shutter: point_shifts has ONE row, evaluated at y = 0; with rolling shutter one row per point, from the point's own y — under horizontal readout too"""
    clip = CLIPS["shifts-r0"]
    pts = [(3.0, 40.0), (100.0, 170.0)]
    one = ZS.point_shifts(clip, clip._stabs[0], pts)
    assert one.shape == (1, 5)
    rolling = clip.with_mode(readout=12.0)
    assert np.array_equal(one[0], ZS.point_shifts(rolling, clip._stabs[0], [(55.0, 0.0)])[0])
    per_point = ZS.point_shifts(rolling, clip._stabs[0], pts)
    assert per_point.shape == (2, 5) and not np.array_equal(per_point[0], per_point[1])
    assert np.array_equal(per_point, ZS.point_shifts(clip.with_mode(readout=12.0, horizontal=True), clip._stabs[0], pts))
    assert ZS.point_shifts(clip.with_mode(2), clip._stabs[0], pts) is None and ZS.point_shifts(clip, None, pts) is None
    assert np.all(ZS.point_shifts(clip, clip._stabs[4], pts) == 0.0)             # unevaluable splines: zeros, not None
