"""gfw_undistort_clip_lens on the MI355X: a clip whose LENS moves from frame to frame (get_lens_data_at_timestamp: a zoom lens's interpolated profile, per-frame
lens telemetry; a keyframed refraction coefficient; mesh_correction[frame]) leaves in shared launches of the moving-lens flavour of the specialised kernel, every
frame bit-exact against the oracle fed that frame's own params and mesh and against gfw_undistort_frame run frame by frame with GFW_OPT_JIT = 0."""
import ctypes as C
import time

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
from _shapes import lens_for
from test_gpu_parity import assert_plane_equal
from test_gpu_fullsize import _View
from test_gpu_lens_models import PHYSICAL, synthetic_mesh

pytestmark = pytest.mark.gpu

W, H = 320, 192
ERR_BUFFER_SIZE_MISMATCH = -8


def zoom_lens(f, n=12, **more):
    """frame f of a zoom-lens clip: the focal length runs from 0.47 W to 0.62 W, the principal point wanders by a few pixels, all four k move"""
    t = f / max(n - 1, 1)
    lens = S.gopro_style_lens(W, H)
    fl = (0.47 + 0.15 * t) * W
    lens["f"] = (fl, fl * (1.0 + 0.004 * t))
    lens["c"] = (W / 2.0 + 0.75 * f - 4.0, H / 2.0 - 0.5 * f + 2.5)
    lens["k"] = [0.045 + 0.006 * f, 0.02 - 0.003 * f, -0.02 + 0.002 * f, 0.006 - 0.0007 * f] + [0.0] * 8
    lens.update(more)
    return lens


def clip(n, lens=zoom_lens, fov=lambda f: 1.1, t2=lambda f: (0.0, 0.0), overrides=None, fill=(), fmt="YUV422P16LE", flags=0, seed=0x1E10, pixels=False, **kw):
    frames = []
    for f in range(n):
        base = dict(overrides(f) if overrides else {})
        base["translation2d"] = t2(f)
        frames.append(S.SyntheticFrame(fmt, W, H, seed=seed + f, timestamp_ms=1000.0 + 33.3 * f, fov=fov(f), base_overrides=base, pixels=pixels,
                                       flags=flags | (abi.FLAG_FILL_WITH_BACKGROUND if f in fill else 0), lens=lens(f), **kw))
    return frames


def mesh_of_frame(f, with_fpd=True, with_mesh=True):
    """synthetic_mesh with its coefficients scaled by the frame index (the cubic terms of the mesh rows, the focal-plane-distortion terms)"""
    m = synthetic_mesh(W, H, with_fpd, with_mesh).copy()
    s = np.float32(1.0 + 0.25 * f)
    o = int(m[0])
    if with_mesh:
        n, base = 9, 9 + 9 * 9 * 2
        for comp in range(2):
            for j in range(n):
                rb = base + comp * n * n * 4 + j * n * 4
                m[rb + 2 * n:rb + 4 * n] *= s
    if with_fpd:
        m[o + 4:o + 20] *= s
    return m


class Device:
    """the frames' planes, outputs and packed tables on the device, and what the calls take of them"""

    def __init__(self, frames):
        import torch
        self.dev = torch.device("cuda", 0)
        self.frames = frames
        self.d_src = [fr.device_planes(self.dev) for fr in frames]
        self.d_dst = [fr.device_outputs(self.dev) for fr in frames]
        self.d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(self.dev) for fr in frames]
        self.d_sums = torch.zeros(len(frames), dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self.types = [pl["pixel_type"] for pl in frames[0].planes]
        self.params = [[pl["params"] for pl in fr.planes] for fr in frames]
        self.bufs = [[warp.device_buffers(self.d_src[j][p].data_ptr(), self.d_src[j][p].numel(), pl["size"], self.d_dst[j][p].data_ptr(), self.d_dst[j][p].numel(), pl["out_size"])
                      for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
        self.rows = frames[0].matrices.shape[0]
        self.mats = [m.data_ptr() for m in self.d_mat]

    def backend(self, jit_mode, synchronous=0):
        import torch
        be = warp.Backend(self.params[0][0], self.types[0], self.frames[0].model, self.frames[0].digital, self.bufs[0][0])
        be.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, synchronous)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        be.set_option(abi.OPT_JIT, jit_mode)
        be.set_option(abi.OPT_PROFILE, 1)
        return be

    def outs(self):
        return [[t.cpu().numpy() for t in d] for d in self.d_dst]

    def srcs(self):
        return [[t.cpu().numpy() for t in d] for d in self.d_src]


def frame_by_frame(be, D, meshes):
    for j in range(len(D.frames)):
        call = warp.FrameCall(be, D.bufs[j], D.params[j], D.types, D.mats[j], D.rows)
        m = None if meshes is None or meshes[j] is None else np.ascontiguousarray(meshes[j], dtype=np.float32)
        rc = call.fn(be.ctx, call.n, call.barr, call.parr, call.tarr, call.mp, call.mc, m.ctypes.data if m is not None else None, m.size if m is not None else 0)
        be._check(rc)


def run(frames, meshes, jit_mode, how, sums=False, wait_ready=False):
    """frames through HIP_DEVICE buffers and packed device tables on one context: "lens" gfw_undistort_clip_lens, "params" gfw_undistort_clip_params (no meshes),
    "frames" gfw_undistort_frame frame by frame, each with its mesh.  -> dict(backend, status, launches, covered, outs, srcs, sums)"""
    import torch
    D = Device(frames)
    be = D.backend(jit_mode)
    try:
        if sums:
            be.set_frame_checksums(D.d_sums.data_ptr(), len(frames))
        if how == "lens":
            warp.ClipLensCall(be, D.bufs, D.params, D.types, D.mats, D.rows, meshes=meshes)()
        elif how == "params":
            assert meshes is None
            warp.ClipParamsCall(be, D.bufs, D.params, D.types, D.mats, D.rows)()
        else:
            frame_by_frame(be, D, meshes)
        be.synchronize()
        backend, status = warp.Backend.last_backend_of(be), be.jit_status()
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
    torch.cuda.synchronize(D.dev)
    return dict(backend=backend, status=status, launches=launches, covered=covered, outs=D.outs(), srcs=D.srcs(),
                sums=[int(v) & 0xFFFFFFFFFFFFFFFF for v in D.d_sums.cpu().numpy().tolist()])


def oracle(fr, src, mesh):
    """the oracle's planes of the frame on the sources the device run read, fed the frame's own params and mesh"""
    v = _View(fr, src)
    if mesh is None:
        return O.run_frame(v)
    ref = []
    for pl in v.planes:
        dst = pl["dst"].copy()
        assert O.undistort_image(pl["src"], pl["size"], dst, pl["out_size"], pl["params"], pl["pixel_type"], fr.model, fr.digital, fr.matrices, mesh=mesh) == 1
        ref.append(dst)
    return ref


def same_as_oracle(frames, meshes, got, what):
    for j, fr in enumerate(frames):
        ref = oracle(fr, got["srcs"][j], None if meshes is None else meshes[j])
        for p, (a, b) in enumerate(zip(ref, got["outs"][j])):
            assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "%s, frame %d plane %d" % (what, j, p))


def check(frames, meshes=None, jit_mode=2, sums=False):
    """the clip call and the frame-by-frame run with GFW_OPT_JIT = 0, both against the oracle (the sources are seeded: both runs read the same bytes)"""
    got = run(frames, meshes, jit_mode, "lens", sums=sums)
    fbf = run(frames, meshes, 0, "frames", sums=sums)
    same_as_oracle(frames, meshes, got, "clip_lens")
    same_as_oracle(frames, meshes, fbf, "frame by frame")
    return got, fbf


def test_a_zoom_lens_clip_shares_one_launch_and_matches_the_oracle():
    frames = clip(12)
    assert len({(tuple(fr.planes[0]["params"].f), tuple(fr.planes[0]["params"].k)) for fr in frames}) == 12
    got, _ = check(frames)
    assert got["backend"].endswith("_jit") and got["status"][0] == 2, (got["backend"], got["status"])
    assert got["covered"] == 12 and got["launches"] < 12, (got["launches"], got["covered"])
    assert got["launches"] == 1, got["launches"]
    assert not np.array_equal(got["outs"][0][0], got["outs"][11][0])


@pytest.mark.parametrize("fmt", ["NV12", "YUV422P16LE"])
@pytest.mark.parametrize("with_mesh,with_fpd", [(True, False), (True, True), (False, True)])
def test_per_frame_meshes_share_launches(fmt, with_mesh, with_fpd):
    frames = clip(12, lens=lambda f: S.gopro_style_lens(W, H), fmt=fmt)
    meshes = [mesh_of_frame(f, with_fpd, with_mesh) for f in range(12)]
    got, _ = check(frames, meshes)
    assert got["backend"].endswith("_jit"), got["backend"]
    assert got["covered"] == 12 and got["launches"] < 12, (got["launches"], got["covered"])


def test_lens_mesh_and_the_per_frame_fields_all_move_at_once():
    frames = clip(12, fov=lambda f: 1.0 + 0.02 * f, t2=lambda f: (-9.5 + 1.75 * f, 6.25 - 1.25 * f), fill=(4,), background_rgba=(0.1, 0.7, 0.3, 1.0),
                  overrides=lambda f: {"lens_correction_amount": 0.3 + 0.05 * f}, fmt="NV12")
    pairs = [mesh_of_frame(i) for i in range(6)]
    meshes = [pairs[f // 2] for f in range(12)]                # (two consecutive frames name one mesh: one upload)
    got, _ = check(frames, meshes)
    assert got["backend"].endswith("_jit") and got["covered"] == 12 and got["launches"] < 12, (got["backend"], got["launches"], got["covered"])


def generic_lens(model, f):
    lens = dict(lens_for(model, W, H))
    k = PHYSICAL[model] + [0.0] * (12 - len(PHYSICAL[model]))
    lens["k"] = [v if v in (0.0, 1.0) else v * (1.0 + 0.02 * f * (1 if i % 2 else -1)) for i, v in enumerate(k)]
    lens["f"] = tuple(v * (1.0 + 0.015 * f) for v in lens["f"])
    lens["c"] = (lens["c"][0] + 0.5 * f, lens["c"][1] - 0.25 * f)
    return lens


@pytest.mark.parametrize("model", ["gopro", "sony"])
def test_generic_model_clips(model):
    frames = clip(12, lens=lambda f: generic_lens(model, f), fov=lambda f: 1.15, fmt="NV12")
    got, _ = check(frames)
    assert got["backend"].endswith("_jit") and got["covered"] == 12 and got["launches"] < 12, (got["backend"], got["launches"], got["covered"])


def test_default_jit_mode_builds_the_specialised_kernel_during_the_call():
    """GFW_OPT_JIT = 1: the flavour's key blanks the lens, so the three-frame trigger fires under a moving lens"""
    frames = clip(12, seed=0x1E40)
    got = run(frames, None, 1, "lens", wait_ready=True)
    assert got["status"][0] == 2, got["status"]
    same_as_oracle(frames, None, got, "default JIT mode")


@pytest.mark.parametrize("what", ["k_all_zero changes at frame 6", "a mesh on frames 0-5 only", "refraction on frames 0-5 only"])
def test_a_change_in_what_the_kernel_is_compiled_for_splits_the_launch(what):
    meshes, kw = None, {}
    if what.startswith("k_all_zero"):
        kw = dict(lens=lambda f: zoom_lens(f, k=[0.0] * 12) if f < 6 else zoom_lens(f))
    elif what.startswith("a mesh"):
        meshes = [mesh_of_frame(f) if f < 6 else None for f in range(12)]
    else:
        kw = dict(overrides=lambda f: {"light_refraction_coefficient": 1.2 + 0.02 * f if f < 6 else 1.0}, flags=abi.FLAG_ANY_UNDERWATER)
    got, _ = check(clip(12, **kw), meshes)
    assert got["covered"] == 12 and 2 <= got["launches"] < 12, (what, got["launches"], got["covered"])


def test_a_constant_lens_call_is_gfw_undistort_clip_params():
    """nothing of the lens moves and no frame has a mesh: the same kernels, the same bits, the certified first pass kept"""
    frames = clip(12, lens=lambda f: S.gopro_style_lens(W, H), fov=lambda f: 1.0 + 0.02 * f, t2=lambda f: (-9.5 + 1.75 * f, 6.25 - 1.25 * f))
    a = run(frames, None, 2, "lens", sums=True)
    b = run(frames, None, 2, "params", sums=True)
    assert a["backend"] == b["backend"] and b["backend"].endswith("_jit"), (a["backend"], b["backend"])
    assert (a["status"][0], a["status"][2]) == (b["status"][0], b["status"][2]) and a["status"][0] == 2
    assert a["sums"] == b["sums"] and all(a["sums"]) and (a["launches"], a["covered"]) == (b["launches"], b["covered"])
    for x, y in zip(a["outs"], b["outs"]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    same_as_oracle(frames, None, a, "constant lens")
    # the same with an array of absent meshes
    import torch
    D = Device(frames)
    be = D.backend(2)
    try:
        call = warp.ClipLensCall(be, D.bufs, D.params, D.types, D.mats, D.rows, meshes=[None] * 12)
        call()
        be.synchronize()
        assert warp.Backend.last_backend_of(be) == b["backend"]
    finally:
        be.close()
    torch.cuda.synchronize(D.dev)
    for x, y in zip(D.outs(), b["outs"]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


def test_twenty_frames_are_dealt_evenly_over_two_launches():
    frames = clip(20, lens=lambda f: zoom_lens(f, 20))
    assert 20 > abi.load_library().gfw_debug_frames_per_launch(0, 0, 0)       # (GFW_CLIP_FRAMES_MAX)
    got, _ = check(frames)
    assert got["covered"] == 20 and got["launches"] == 2, (got["launches"], got["covered"])


def test_two_asynchronous_calls_back_to_back_keep_their_own_staging():
    """an asynchronous context, two calls with no synchronise between: the second call's lens slots and meshes must not disturb what the first's launch reads"""
    import torch
    first = clip(12, lens=lambda f: S.gopro_style_lens(W, H), fmt="NV12", seed=0x1E60)
    second = clip(12, lens=lambda f: zoom_lens(11 - f), fmt="NV12", seed=0x1E80)
    m1 = [mesh_of_frame(f) for f in range(12)]
    m2 = [mesh_of_frame(20 - f) for f in range(12)]
    D1, D2 = Device(first), Device(second)
    be = D1.backend(2)
    try:
        c1 = warp.ClipLensCall(be, D1.bufs, D1.params, D1.types, D1.mats, D1.rows, meshes=m1)
        c2 = warp.ClipLensCall(be, D2.bufs, D2.params, D2.types, D2.mats, D2.rows, meshes=m2)
        c1()
        c2()
        be.synchronize()
        _, launches, covered = be.get_profile_frames()
    finally:
        be.close()
    torch.cuda.synchronize(D1.dev)
    assert covered == 24 and launches < 24, (launches, covered)
    same_as_oracle(first, m1, dict(outs=D1.outs(), srcs=D1.srcs()), "first call")
    same_as_oracle(second, m2, dict(outs=D2.outs(), srcs=D2.srcs()), "second call")


def test_without_the_specialised_kernel_frames_go_one_by_one():
    """GFW_OPT_JIT = 0: the ahead-of-time kernels, frame by frame"""
    frames = clip(12, fmt="NV12")
    meshes = [mesh_of_frame(f) if f % 2 else None for f in range(12)]
    got = run(frames, meshes, 0, "lens")
    assert not got["backend"].endswith("_jit") and got["launches"] == 12 and got["covered"] == 12, (got["backend"], got["launches"], got["covered"])
    same_as_oracle(frames, meshes, got, "GFW_OPT_JIT = 0")


def test_host_buffers_are_served_per_frame():
    frames = clip(4, lens=lambda f: zoom_lens(f, 4), fmt="NV12", pixels=True)
    meshes = [mesh_of_frame(f) for f in range(4)]
    outs = [[pl["dst"].copy() for pl in fr.planes] for fr in frames]
    bufs = [[warp.host_buffers(pl["src"], pl["size"], o, pl["out_size"]) for pl, o in zip(fr.planes, outs[j])] for j, fr in enumerate(frames)]
    params = [[pl["params"] for pl in fr.planes] for fr in frames]
    types = [pl["pixel_type"] for pl in frames[0].planes]
    be = warp.Backend(params[0][0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    try:
        be.set_option(abi.OPT_JIT, 2)
        be.set_option(abi.OPT_PROFILE, 1)
        warp.ClipLensCall(be, bufs, params, types, [fr.matrices for fr in frames], meshes=meshes)()
        be.synchronize()
        _, launches, covered = be.get_profile_frames()
    finally:
        be.close()
    assert (launches, covered) == (4, 4), (launches, covered)
    for j, fr in enumerate(frames):
        for p, (a, b) in enumerate(zip(oracle(fr, [pl["src"] for pl in fr.planes], meshes[j]), outs[j])):
            assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "host buffers, frame %d plane %d" % (j, p))


def test_frame_checksums_are_those_of_the_frame_by_frame_run():
    frames = clip(12, fill=(3,), background_rgba=(0.2, 0.4, 0.6, 1.0))
    got, fbf = check(frames, sums=True)
    assert got["sums"] == fbf["sums"] and all(s != 0 for s in got["sums"]), (got["sums"], fbf["sums"])
    meshes = [mesh_of_frame(f) for f in range(12)]
    got, fbf = check(clip(12, fmt="NV12"), meshes, sums=True)
    assert got["sums"] == fbf["sums"] and all(s != 0 for s in got["sums"]), (got["sums"], fbf["sums"])


def test_rejected_arguments_write_nothing_and_name_the_frame():
    import torch
    frames = clip(3)
    D = Device(frames)
    before = [[t.clone() for t in d] for d in D.d_dst]
    be = D.backend(2)
    try:
        good = [mesh_of_frame(f) for f in range(3)]
        call = warp.ClipLensCall(be, D.bufs, D.params, D.types, D.mats, D.rows, meshes=good)
        fn, err = be.lib.gfw_undistort_clip_lens, be.lib.gfw_last_error

        def lens_call(n=3, mc=call.mc, ptrs=call.mesh_ptrs, lens=call.mesh_lens):
            return fn(be.ctx, n, call.n, call.barr, call.parr, call.tarr, call.marr, mc, ptrs, lens)

        assert lens_call(n=-1) == abi.ERR_INVALID_ARGUMENT
        assert lens_call(mc=-1) == abi.ERR_INVALID_ARGUMENT
        assert lens_call(ptrs=None) == abi.ERR_INVALID_ARGUMENT and b"mesh_lens without meshes" in err()
        no_ptr = (C.c_void_p * 3)(call.mesh_ptrs[0], None, call.mesh_ptrs[2])
        assert lens_call(ptrs=no_ptr) == abi.ERR_INVALID_ARGUMENT and b"frame 1" in err()
        too_long = (C.c_size_t * 3)(839, 840, 839)
        assert lens_call(lens=too_long) == ERR_BUFFER_SIZE_MISMATCH and b"frame 1" in err()
        bad = good[2].copy()
        bad[1] = 1.0                                             # a 1 x 9 grid: outside 2..9
        bad_ptrs = (C.c_void_p * 3)(call.mesh_ptrs[0], call.mesh_ptrs[1], bad.ctypes.data)
        assert lens_call(ptrs=bad_ptrs) == ERR_BUFFER_SIZE_MISMATCH and b"frame 2" in err() and b"grid" in err()
        offset = good[1].copy()
        offset[0] = 5000.0                                       # the focal-plane block's offset beyond the block
        off_ptrs = (C.c_void_p * 3)(call.mesh_ptrs[0], offset.ctypes.data, call.mesh_ptrs[2])
        assert lens_call(ptrs=off_ptrs) == ERR_BUFFER_SIZE_MISMATCH and b"frame 1" in err()
        assert lens_call(n=0) == 0
        be.synchronize()
        _, launches, covered = be.get_profile_frames()
        assert (launches, covered) == (0, 0), (launches, covered)
    finally:
        be.close()
    torch.cuda.synchronize(D.dev)
    for a, b in zip(before, D.d_dst):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
