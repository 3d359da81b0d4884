"""gfw_undistort_clip_params on the MI355X: a clip whose KernelParams move from frame to frame (FrameTransform::at_timestamp — the adaptive-zoom fov and its
centre, keyframed lens correction, background margin and feather; the render loop's fill flag) leaves in shared launches of the per-frame flavour of the
specialised kernel, every frame bit-exact against the oracle fed that frame's own params and against gfw_undistort_frame run frame by frame."""
import ctypes as C
import time

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
from test_gpu_parity import assert_plane_equal
from test_gpu_fullsize import _View

pytestmark = pytest.mark.gpu

W, H = 320, 192


def clip(n, fov=lambda f: 1.0 + 0.02 * f, t2=lambda f: (-9.5 + 1.75 * f, 6.25 - 1.25 * f), overrides=None, fill=(), fmt="YUV422P16LE", lens=None, seed=0x5E10, **kw):
    frames = []
    for f in range(n):
        base = dict(overrides(f) if overrides else {})
        base["translation2d"] = t2(f)
        frames.append(S.SyntheticFrame(fmt, W, H, seed=seed + f, timestamp_ms=1000.0 + 33.3 * f, fov=fov(f), base_overrides=base, pixels=False,
                                       flags=abi.FLAG_FILL_WITH_BACKGROUND if f in fill else 0, lens=lens(f) if lens else None, **kw))
    return frames


def run(frames, jit_mode, use_clip, sums=False, wait_ready=False):
    """frames through HIP_DEVICE buffers and packed device tables on one context: gfw_undistort_clip_params (use_clip), or gfw_undistort_frame frame by frame.
    -> dict(backend, status, launches, covered, outs, srcs, sums)"""
    import torch
    dev = torch.device("cuda", 0)
    d_src = [fr.device_planes(dev) for fr in frames]
    d_dst = [fr.device_outputs(dev) for fr in frames]
    d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
    d_sums = torch.zeros(len(frames), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [[pl["params"] for pl in fr.planes] for fr in frames]
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(), d_dst[j][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
    rows = frames[0].matrices.shape[0]
    be = warp.Backend(params[0][0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    try:
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        be.set_option(abi.OPT_JIT, jit_mode)
        be.set_option(abi.OPT_PROFILE, 1)
        if sums:
            be.set_frame_checksums(d_sums.data_ptr(), len(frames))
        if use_clip:
            warp.ClipParamsCall(be, bufs, params, types, [m.data_ptr() for m in d_mat], rows)()
        else:
            for j in range(len(frames)):
                warp.FrameCall(be, bufs[j], params[j], types, d_mat[j].data_ptr(), rows)()
        be.synchronize()
        backend, status = warp.last_backend(), be.jit_status()
        _, launches, covered = be.get_profile_frames()
        if wait_ready:
            deadline = time.time() + 90.0
            while status[0] == 1 and time.time() < deadline:
                time.sleep(0.25)
                status = be.jit_status()
        if sums:
            be.set_frame_checksums(0, 0)
    finally:
        be.close()
    torch.cuda.synchronize(dev)
    return dict(backend=backend, status=status, launches=launches, covered=covered, outs=[[t.cpu().numpy() for t in d] for d in d_dst],
                srcs=[[t.cpu().numpy() for t in d] for d in d_src], sums=[int(v) & 0xFFFFFFFFFFFFFFFF for v in d_sums.cpu().numpy().tolist()])


def check(frames, jit_mode=2, sums=False):
    got = run(frames, jit_mode, True, sums=sums)
    fbf = run(frames, 0, False, sums=sums)
    for j, fr in enumerate(frames):
        ref = O.run_frame(_View(fr, got["srcs"][j]))
        for p, (a, b, c) in enumerate(zip(ref, got["outs"][j], fbf["outs"][j])):
            assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "clip_params, frame %d plane %d" % (j, p))
            assert_plane_equal(a, c, fr.planes[p]["pixel_type"], "frame by frame, frame %d plane %d" % (j, p))
    return got, fbf


def test_dynamic_zoom_clip_shares_launches_and_matches_the_oracle():
    frames = clip(12)
    got, _ = check(frames)
    assert got["backend"].endswith("_jit") and got["status"][0] == 2, (got["backend"], got["status"])
    assert got["covered"] == 12 and got["launches"] < 12, (got["launches"], got["covered"])


def test_default_jit_mode_builds_the_specialised_kernel_during_the_call():
    """GFW_OPT_JIT = 1: the per-frame flavour's key blanks the moving fields, so the three-frame trigger fires under a moving zoom centre"""
    frames = clip(12, seed=0x5E40)
    got = run(frames, 1, True, wait_ready=True)
    assert got["status"][0] == 2, got["status"]
    for j, fr in enumerate(frames):
        for p, (a, b) in enumerate(zip(O.run_frame(_View(fr, got["srcs"][j])), got["outs"][j])):
            assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "default JIT mode, frame %d plane %d" % (j, p))


@pytest.mark.parametrize("what,kw", [
    ("keyframed lens correction", dict(overrides=lambda f: {"lens_correction_amount": 0.3 + 0.6 * f / 11.0})),
    ("margin and feather", dict(fov=lambda f: 1.2 + 0.02 * f, overrides=lambda f: {"background_mode": 3, "background_margin": 0.04 + 0.01 * f,
                                                                                     "background_margin_feather": 0.15 - 0.01 * f}, background_rgba=(0.8, 0.2, 0.4, 1.0))),
    ("fill on frames 0, 5, 11", dict(fill=(0, 5, 11), background_rgba=(0.1, 0.7, 0.3, 1.0))),
    ("NV12 dynamic zoom", dict(fmt="NV12")),
    ("RGBA dynamic zoom", dict(fmt="RGBA")),
])
def test_per_frame_fields_share_launches(what, kw):
    frames = clip(12, **kw)
    got, _ = check(frames)
    assert got["backend"].endswith("_jit"), (what, got["backend"])
    assert got["covered"] == 12 and got["launches"] < 12, (what, got["launches"], got["covered"])


def test_a_clip_constant_change_mid_call_splits_the_launch():
    base = S.gopro_style_lens(W, H)
    other = dict(base, k=[0.05, 0.01, -0.02, 0.006] + [0.0] * 8)
    got, _ = check(clip(12, lens=lambda f: base if f < 6 else other))
    assert got["launches"] >= 2 and got["launches"] < 12, got["launches"]
    got, _ = check(clip(12, overrides=lambda f: {"lens_correction_amount": 0.5 if f < 6 else 1.0}))
    assert got["launches"] >= 2 and got["launches"] < 12, got["launches"]


def test_a_wide_zoom_range_is_covered_by_the_tables_envelope():
    """the last frame's corner rays lie well beyond the first frame's: a table sized for frame 0 alone would not cover it"""
    got, _ = check(clip(12, fov=lambda f: 0.7 + 0.15 * f, t2=lambda f: (-20.0 + 4.0 * f, 12.0 - 2.5 * f)))
    assert got["launches"] < 12, got["launches"]


def test_frame_checksums_are_those_of_the_frame_by_frame_run():
    got, fbf = check(clip(12, fill=(3,)), sums=True)
    assert got["sums"] == fbf["sums"] and all(s != 0 for s in got["sums"]), (got["sums"], fbf["sums"])


def test_argument_errors_write_nothing():
    import torch
    dev = torch.device("cuda", 0)
    frames = clip(2)
    d_src = [fr.device_planes(dev) for fr in frames]
    d_dst = [fr.device_outputs(dev) for fr in frames]
    d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
    before = [[t.clone() for t in d] for d in d_dst]
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [[pl["params"] for pl in fr.planes] for fr in frames]
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(), d_dst[j][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
    be = warp.Backend(params[0][0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    try:
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        call = warp.ClipParamsCall(be, bufs, params, types, [m.data_ptr() for m in d_mat], frames[0].matrices.shape[0])
        fn = be.lib.gfw_undistort_clip_params
        assert fn(be.ctx, 2, call.n, call.barr, None, call.tarr, call.marr, call.mc) == abi.ERR_INVALID_ARGUMENT
        assert fn(be.ctx, -1, call.n, call.barr, call.parr, call.tarr, call.marr, call.mc) == abi.ERR_INVALID_ARGUMENT
        bad = (C.c_int * call.n)(*([99] + list(call.tarr)[1:]))
        assert fn(be.ctx, 2, call.n, call.barr, call.parr, bad, call.marr, call.mc) == abi.ERR_INVALID_ARGUMENT
        assert b"pixel type" in be.lib.gfw_last_error()
        be.synchronize()
    finally:
        be.close()
    torch.cuda.synchronize(dev)
    for a, b in zip(before, d_dst):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
