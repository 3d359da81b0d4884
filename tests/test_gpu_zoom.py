"""gfw_zoom_fovs on the MI355X: FovIterative::find_fov of a whole clip in one device call, against the host statement (tests/_zoomstmt.py).

Caller-given rotations: bit-identical fov_minimal and debug polygon.  Rotations from the tracks: the device's f64 acos / sin are the device library's, the
statement's the host libm's, so an f32 entry of a point's `new_k * R` can differ in its last bits (the standing bar of that stage: <= 2 ULP,
tests/test_gpu_matrix_builder.py); the tolerance is TWICE the per-clip maximum that tests/golden/zoom_rotation_sensitivity.py measured with the statement alone
for rotations displaced by -2 .. +2 ULP (tests/golden/zoom_rotation_sensitivity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp, zooming
import _oracle as O
import _zoomstmt as Z
import _zoomcase as ZC
from test_gpu_parity import assert_plane_equal
from test_gpu_fullsize import _View

pytestmark = pytest.mark.gpu

CLIPS = {c.name: c for c in Z.statement_clips()}
SENS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoom_rotation_sensitivity.json")))["clips"]


def backend_for(clip):
    fr = S.SyntheticFrame("NV12", clip.size[0], clip.size[1], seed=3, lens=clip.lens, pixels=True)
    pl = fr.planes[0]
    b = warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"])
    return warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, b)


def same_f64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_given_rotations_bit_identical(name):
    """host and device output, synchronous and asynchronous context, 1 / 24 / 5000 frames (the 24 tiled)"""
    import torch
    dev = torch.device("cuda", 0)
    clip = ZC.readout0(CLIPS[name])
    ref_f, ref_d = Z.clip_fovs(clip, given_rotations=True)
    assert np.all(np.isfinite(ref_f)) and np.all(ref_f > 0.3) and np.all(ref_f < 3.0)
    be = backend_for(clip)
    try:
        kp, search, frames, rot = ZC.inputs(clip, True)
        fov, dbg = be.zoom_fovs(kp, search, frames, rotations=rot, debug=True)
        assert warp.last_backend() == "zoom_fovs"
        assert same_f64(fov, ref_f), (name, np.max(np.abs(fov - ref_f)))
        assert same_f64(dbg, ref_d), name
        one = (abi.ZoomFrame * 1)(frames[5])
        assert same_f64(be.zoom_fovs(kp, search, one, rotations=rot[5:6]), ref_f[5:6])
        tile = 209                                                                              # 5016 frames: the first 5000 go
        kp, search, frames, rot = ZC.inputs(clip, True, tile=tile)
        n = 5000
        many = (abi.ZoomFrame * n).from_buffer(frames)
        big_f, big_d = np.tile(ref_f, tile)[:n], np.tile(ref_d, (tile, 1, 1))[:n]
        d_f = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        d_d = torch.full((n, 120, 2), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        assert be.zoom_fovs(kp, search, many, rotations=rot[:n], out_ptr=d_f.data_ptr(), debug_ptr=d_d.data_ptr()) is None       # synchronous context, device output
        assert same_f64(d_f.cpu().numpy(), big_f) and same_f64(d_d.cpu().numpy(), big_d), name
        d_f.fill_(-1.0)
        torch.cuda.synchronize(dev)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.zoom_fovs(kp, search, many, rotations=rot[:n], out_ptr=d_f.data_ptr())                                                  # asynchronous: in order on the stream
        be.zoom_fovs(kp, search, (abi.ZoomFrame * 24).from_buffer(frames), rotations=rot[:24], out_ptr=d_f.data_ptr())            # ... and a second call behind it
        be.synchronize()
        assert same_f64(d_f.cpu().numpy(), big_f), name
        assert same_f64(be.zoom_fovs(kp, search, many, rotations=rot[:n]), big_f), name                                            # asynchronous context, host output
    finally:
        be.close()


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_rotations_from_tracks_within_the_measured_sensitivity(name):
    clip = CLIPS[name]
    ref_f, ref_d = Z.clip_fovs(clip)
    be = backend_for(clip)
    try:
        be.set_quaternion_tracks(*clip.tracks)
        if clip.sync_offsets is not None:
            be.set_sync_offsets(clip.duration_ms, *clip.sync_offsets)
        kp, search, frames, _ = ZC.inputs(clip, False)
        fov, dbg = be.zoom_fovs(kp, search, frames, debug=True)
    finally:
        be.close()
    rel = float(np.max(np.abs(fov - ref_f) / ref_f))
    poly = float(np.max(np.abs(dbg - ref_d)))
    bar_f, bar_p = 2.0 * SENS[name]["fov_max_rel"], 2.0 * SENS[name]["polygon_max_abs"]
    print("%s: fov_minimal relative difference %.3g (bar %.3g), polygon %.3g (bar %.3g), %d of %d frames bit-identical"
          % (name, rel, bar_f, poly, bar_p, int(np.sum(fov == ref_f)), len(fov)))
    assert rel <= bar_f, (name, rel, bar_f)
    assert poly <= bar_p, (name, poly, bar_p)


def test_arguments():
    import torch
    clip = ZC.readout0(CLIPS["fisheye-320x180-r0-l1-c0"])
    kp, search, frames, rot = ZC.inputs(clip, True)
    be = backend_for(clip)
    lib = be.lib
    f = lib.gfw_zoom_fovs
    out = np.full(24, -7.0)
    fp, rp, op = C.cast(frames, C.c_void_p), rot.ctypes.data, out.ctypes.data
    INV = abi.ERR_INVALID_ARGUMENT
    try:
        assert f(be.ctx, C.byref(kp), C.byref(search), fp, 0, rp, op, None, 0) == 0 and np.all(out == -7.0)          # n_frames = 0: success, nothing written
        assert f(be.ctx, C.byref(kp), C.byref(search), None, 0, None, None, None, 0) == 0
        for args in ((None, C.byref(kp), C.byref(search), fp, 24, rp, op, None, 0), (be.ctx, None, C.byref(search), fp, 24, rp, op, None, 0),
                     (be.ctx, C.byref(kp), None, fp, 24, rp, op, None, 0), (be.ctx, C.byref(kp), C.byref(search), None, 24, rp, op, None, 0),
                     (be.ctx, C.byref(kp), C.byref(search), fp, 24, rp, None, None, 0), (be.ctx, C.byref(kp), C.byref(search), fp, -1, rp, op, None, 0)):
            assert f(*args) == INV and lib.gfw_last_error()
        assert f(be.ctx, C.byref(kp), C.byref(search), fp, 24, None, op, None, 0) == INV and b"tracks" in lib.gfw_last_error()     # no tracks, no rotations
        frames[3].frame_readout_time_ms = 8.0
        assert f(be.ctx, C.byref(kp), C.byref(search), fp, 24, rp, op, None, 0) == INV and b"frame 3" in lib.gfw_last_error()      # readout with one rotation per frame
        frames[3].frame_readout_time_ms = 0.0
        frames[7].suppress_rotation = 2
        assert f(be.ctx, C.byref(kp), C.byref(search), fp, 24, rp, op, None, 0) == INV and b"suppress_rotation" in lib.gfw_last_error()
        frames[7].suppress_rotation = 0
        for flag in (abi.FLAG_HAS_IBIS_DATA, abi.FLAG_HAS_MESH_DATA, abi.FLAG_HAS_FPD_DATA):                                      # shifts / mesh clips: not covered
            bad = kp.copy()
            bad.flags |= flag
            assert f(be.ctx, C.byref(bad), C.byref(search), fp, 24, rp, op, None, 0) == INV and b"gfw_undistort_points" in lib.gfw_last_error()
        bad = abi.ZoomSearch.from_buffer_copy(search)
        bad.horizontal_readout = 2
        assert f(be.ctx, C.byref(kp), C.byref(bad), fp, 24, rp, op, None, 0) == INV
        bad = abi.ZoomSearch.from_buffer_copy(search)
        bad.width = 0
        assert f(be.ctx, C.byref(kp), C.byref(bad), fp, 24, rp, op, None, 0) == INV
        bad = abi.ZoomSearch.from_buffer_copy(search)
        bad.org_output_width = 0                                                                                                  # the reference would divide by it
        assert f(be.ctx, C.byref(kp), C.byref(bad), fp, 24, rp, op, None, 0) == INV
        assert np.all(out == -7.0)
        assert f(be.ctx, C.byref(kp), C.byref(search), fp, 24, rp, op, None, 0) == 0 and np.all(out > 0.0)
    finally:
        be.close()
    torch.cuda.synchronize()


def test_calculate_fovs_then_render_end_to_end():
    """zooming.calculate_fovs on a 48-frame 640x360 NV12 fisheye clip with shake (window 1 s, Gaussian filter), then the frames through undistort_clip_params:
    with fov = fovs[f] * 0.97 no pixel of any frame shows background (dynamic fovs are <= the minimal ones: min_rolling, then a normalised non-negative window),
    with fov_minimal[f] * 1.03 every frame does; the pixels bit-exact against the oracle given the same parameters."""
    from test_gpu_clip_params import run
    clip = Z.Clip("e2e", size=(640, 360), out=(640, 360), readout=10.0, center=(0.02, -0.015), frames=48, seed=23)
    clip.timestamps = [1000.0 + 1000.0 / 30.0 * k for k in range(48)]
    cp = ZC.compute_params(clip)
    cp.adaptive_zoom_window, cp.scaled_fps = 1.0, 30.0
    be = backend_for(clip)
    try:
        be.set_quaternion_tracks(*clip.tracks)
        fovs, minimal = zooming.calculate_fovs(cp, list(enumerate(clip.timestamps)), zooming.GAUSSIAN_FILTER, be)
        assert warp.last_backend() == "zoom_fovs"
    finally:
        be.close()
    assert len(fovs) == 48 and np.all(fovs <= minimal * (1.0 + 1e-12)) and np.ptp(minimal) > 0.01
    ref_min, _ = Z.clip_fovs(clip)
    assert np.max(np.abs(minimal - ref_min) / ref_min) < 1e-5
    assert fovs.tolist() == Z.zoom_smooth(minimal, 1.0, 30.0, 0)[0]
    for series, scale, want_background in ((fovs, 0.97, False), (minimal, 1.03, True)):
        outs = []
        for bg in (0.0, 1.0):
            frames = [ZC.render_frame(clip, k, series[k] * scale, bg, pixels=False, seed=0x700 + k) for k in range(48)]
            got = run(frames, 2, True)
            assert got["backend"].startswith("yuv_fused"), got["backend"]
            for j, fr in enumerate(frames):
                for p, (a, b) in enumerate(zip(O.run_frame(_View(fr, got["srcs"][j])), got["outs"][j])):
                    assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "zoomed clip x%.2f, frame %d plane %d" % (scale, j, p))
            outs.append(got["outs"])
        for j in range(48):
            differ = sum(int(np.count_nonzero(a != b)) for a, b in zip(outs[0][j], outs[1][j]))
            assert (differ > 0) == want_background, (scale, j, differ)
