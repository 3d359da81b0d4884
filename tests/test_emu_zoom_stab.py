"""The kernels of gfw_zoom_fovs_stab (gfw_zoom.hip: gfw_zoom_stab_kernel), interpreted on the host (tests/_zoomstab.py, tests/emu/emu_zoom_stab_driver.inc),
against the host statement with per-point IBIS/OIS shifts and per-frame meshes.

Bit-identical wherever no track is read: caller-given rotations (no rolling shutter), and suppress_rotation 1 and 2 with rolling shutter in both readout
directions — the rotation is new_k alone on either side, while the shifts still follow each point's own y (suppress_rotation 2 drops them).  With rotations from
the tracks the bar is the project's: twice the effect of a -2 .. +2 ULP displacement of every f32 rotation entry in the statement
(tests/golden/zoom_stab_sensitivity.json, measured by tests/golden/zoom_stab_sensitivity.py as zoom_rotation_sensitivity.json was).

The clips (_zoomstab.stab_clips): frames with and without a camera_stab_data entry in one call, one frame whose splines cannot be evaluated (a shift of zeros,
which is not no shift); shifts only, mesh only, the focal-plane-distortion block only, all three together; the lens-correction blend below 1 with shifts; the
fisheye, two generic models (sony, poly5) and a digital lens; per-frame zoom centres, strengths and time offsets."""
import json
import os

import numpy as np
import pytest

import _zoomstmt as Z
import _zoomstab as ZS
import _zoomcase as ZC
import _emu_zoom as E

CLIPS = {c.name: c for c in ZS.stab_clips()}
SENS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoom_stab_sensitivity.json")))["clips"]


def same_f64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_given_rotations_bit_identical(name):
    clip = CLIPS[name].with_mode(0, readout=0.0)
    fov, dbg = ZS.emu_clip_fovs(clip, given_rotations=True)
    ref_f, ref_d = ZS.clip_fovs(clip, given_rotations=True)
    assert np.all(np.isfinite(ref_f)) and np.all(ref_f > 0.3) and np.all(ref_f < 3.0)
    assert same_f64(fov, ref_f), (name, fov, ref_f)
    assert same_f64(dbg, ref_d), name


@pytest.mark.parametrize("mode,horizontal", [(1, False), (1, True), (2, False), (2, True)])
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_suppressed_rotation_with_rolling_shutter_bit_identical(name, mode, horizontal):
    clip = CLIPS[name].with_mode(mode, readout=12.0, horizontal=horizontal)
    fov, dbg = ZS.emu_clip_fovs(clip)
    ref_f, ref_d = ZS.clip_fovs(clip)
    assert same_f64(fov, ref_f), (name, mode, horizontal, fov, ref_f)
    assert same_f64(dbg, ref_d), (name, mode, horizontal)
    if mode == 2 and CLIPS[name]._meshes is None:                                # the shifts are dropped, the rotation is new_k alone: nothing of the frame's time is left
        assert np.all(ref_f == ref_f[0]) or CLIPS[name].keyframed


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_rotations_from_tracks(name):
    clip = CLIPS[name]
    fov, dbg = ZS.emu_clip_fovs(clip)
    ref_f, ref_d = ZS.clip_fovs(clip)
    rel, poly = float(np.max(np.abs(fov - ref_f) / ref_f)), float(np.max(np.abs(dbg - ref_d)))
    print("%s: fov_minimal relative difference %.3g (bar %.3g), polygon %.3g (bar %.3g)" % (name, rel, 2.0 * SENS[name]["fov_max_rel"], poly, 2.0 * SENS[name]["polygon_max_abs"]))
    assert rel <= 2.0 * SENS[name]["fov_max_rel"], name
    assert poly <= 2.0 * SENS[name]["polygon_max_abs"], name


def test_without_rolling_shutter_only_index_zero_is_shifted():
    """points_iter is the single point (0, 0): shift_per_point holds ONE shift and `.get(index)` hands it to point 0 of each mapped set only.  The interpreted kernel
    equals the statement as written; shifting every point (what the code reads like it meant) gives other results, and the first polygon shows exactly which points moved."""
    clip = CLIPS["shifts-r0"].with_mode(0, readout=0.0)
    fov, dbg = ZS.emu_clip_fovs(clip, given_rotations=True)
    ref_f, ref_d = ZS.clip_fovs(clip, given_rotations=True)
    all_f, all_d = ZS.clip_fovs(clip, given_rotations=True, shift_every_point=True)
    plain_f, plain_d = Z.clip_fovs(clip, given_rotations=True)
    assert same_f64(fov, ref_f) and same_f64(dbg, ref_d)
    real = [k for k in range(24) if clip._stabs[k] is not None and k != 4]       # frames with an entry whose splines can be evaluated
    for k in real:
        assert not np.array_equal(dbg[k, 0], plain_d[k, 0]), k                   # outline point 0 carries the shift ...
        assert same_f64(dbg[k, 1:], plain_d[k, 1:]), k                           # ... every other point is the plain clip's
        assert not same_f64(dbg[k, 1:], all_d[k, 1:]), k
    assert sum(fov[k] != all_f[k] for k in real) >= len(real) // 2, (fov, all_f)  # the result does change if all points are shifted
    assert same_f64(dbg[2], plain_d[2]) and fov[2] == plain_f[2]                 # no entry: the plain clip's frame


def test_null_tables_are_the_plain_search():
    clip = CLIPS["shifts-r12"]
    kp, search, frames, _, _, _ = ZS.inputs(clip)
    a = ZS.emu_zoom_fovs(kp, clip.model, clip.digital, search, frames, tracks=clip.tracks)
    b = E.zoom_fovs(kp, clip.model, clip.digital, search, frames, tracks=clip.tracks)
    assert same_f64(a[0], b[0]) and same_f64(a[1], b[1])
    # a table whose every entry is absent runs the stabiliser kernel and gives the same bits: no entry is no shift
    c = ZS.emu_zoom_fovs(kp, clip.model, clip.digital, search, frames, stabs=[None] * 24, meshes=[None] * 24, tracks=clip.tracks)
    assert same_f64(a[0], c[0]) and same_f64(a[1], c[1])
