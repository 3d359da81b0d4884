#!/usr/bin/env python3
"""A 4K 16-bit 4:2:2 zoom-lens clip (C2: fisheye, rolling shutter, bilinear; f, c and k move on every frame — what get_lens_data_at_timestamp hands a render of
a zoom lens or of per-frame lens telemetry) four ways in one process, kernel time per frame from gfw_get_profile_frames and wall time per frame around the calls:
  (a) gfw_undistort_frame frame by frame, GFW_OPT_JIT = 1 (the default: the lens moves every frame, so the constant-lens specialisation never gets its three
      frames and the clip stays on the ahead-of-time kernels),
  (b) gfw_undistort_clip_params (its launches share nothing across a lens change: one launch per frame),
  (c) gfw_undistort_clip_lens (the moving-lens flavour of the specialised kernel, shared launches),
  (d) the same frames with frame 0's lens through gfw_undistort_clip_params — not the same pixels: the floor, (c) against (d) is what the exact first pass and
      the slot loads cost.
--mesh: the clip also has a mesh per frame; (a) and (c) take it, (b) and (d) cannot (gfw_undistort_clip_params has no mesh) and run the mesh-less clip.
The variants alternate, each repeat is printed.  HIP_DEVICE buffers, packed device tables, one context per variant, GFW_OPT_JIT = 2 for (b), (c), (d).
usage: clip_lens_bench.py [--frames N] [--reps R] [--mesh] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402

W, H = 3840, 2160


def zoom_lens(f, n):
    t = f / max(n - 1, 1)
    lens = S.gopro_style_lens(W, H)
    fl = (0.47 + 0.15 * t) * W
    lens["f"] = (fl, fl * (1.0 + 0.004 * t))
    lens["c"] = (W / 2.0 + 0.5 * f - 16.0, H / 2.0 - 0.25 * f + 8.0)
    lens["k"] = [0.045 + 0.0008 * f, 0.02 - 0.0004 * f, -0.02 + 0.0003 * f, 0.006 - 0.0001 * f] + [0.0] * 8
    return lens


def frames_of(n, moving):
    return [S.SyntheticFrame("YUV422P16LE", W, H, seed=0xC1 + f, timestamp_ms=1000.0 + 33.3 * f, fov=1.1, pixels=False, lens=zoom_lens(f if moving else 0, n)) for f in range(n)]


def mesh_of_frame(f):
    """a Sony-style mesh_data block (header, 9 x 9 grid, cubic row coefficients, focal-plane-distortion terms) whose terms grow with the frame index"""
    n = 9
    m = np.zeros(839, dtype=np.float32)
    o = 9 + n * n * 2 + n * n * 4 * 2
    m[0:9] = (o, n, n, W, H, 0.0, 0.0, W, H)
    base, s = 9 + n * n * 2, 1.0 + 0.02 * f
    for comp in range(2):
        for j in range(n):
            rb = base + comp * n * n * 4 + j * n * 4
            for i in range(n):
                if comp == 0:
                    co = (i * W / 8.0 + 1.5 * np.sin(0.7 * i + 0.3 * j), 1.0 + 0.01 * np.cos(i + j), 1e-4 * (i - 4) * s, -1e-7 * (j - 3) * s)
                else:
                    co = (j * H / 8.0 + 1.2 * np.cos(0.5 * i - 0.2 * j), 0.004 * np.sin(i - j), 2e-5 * (j - 4) * s, 1e-8 * (i - 2) * s)
                m[rb + i], m[rb + n + i], m[rb + 2 * n + i], m[rb + 3 * n + i] = co
    m[o] = 1.0
    for idx in range(8):
        m[o + 4 + idx * 2], m[o + 5 + idx * 2] = 0.002 * (idx - 3) * s, -0.001 * (idx - 4) * s
    return m


class FrameByFrame:
    def __init__(self, be, bufs, params, types, mats, rows, meshes):
        self.be = be
        self.calls = [warp.FrameCall(be, bufs[j], params[j], types, mats[j], rows) for j in range(len(bufs))]
        self.meshes = [None if m is None else np.ascontiguousarray(m, dtype=np.float32) for m in (meshes or [None] * len(bufs))]

    def __call__(self):
        for c, m in zip(self.calls, self.meshes):
            rc = c.fn(self.be.ctx, c.n, c.barr, c.parr, c.tarr, c.mp, c.mc, m.ctypes.data if m is not None else None, m.size if m is not None else 0)
            if rc != 0:
                self.be._check(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least three repeats: the spread between repeats is what a difference is judged against")
    dev = torch.device("cuda", 0)
    moving, still = frames_of(a.frames, True), frames_of(a.frames, False)
    meshes = [mesh_of_frame(f) for f in range(a.frames)] if a.mesh else None
    d_src = [fr.device_planes(dev) for fr in moving]
    d_dst = [fr.device_outputs(dev) for fr in moving]
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in moving[0].planes]
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(), d_dst[j][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(moving)]
    rows = moving[0].matrices.shape[0]

    def tables(frames):
        t = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
        return t, [m.data_ptr() for m in t], [[pl["params"] for pl in fr.planes] for fr in frames]

    keep_m, mats_m, params_m = tables(moving)
    keep_s, mats_s, params_s = tables(still)
    torch.cuda.synchronize(dev)
    res = {"clip": "4K YUV422P16LE, fisheye, bilinear, rolling shutter, f 0.47-0.62 W, c and k moving per frame" + (", a mesh per frame" if a.mesh else ""),
           "frames": a.frames, "reps": a.reps, "mesh": bool(a.mesh)}
    backends, variants = [], {}

    def backend(jit):
        be = warp.Backend(params_m[0][0], types[0], moving[0].model, moving[0].digital, bufs[0][0])
        backends.append(be)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        be.set_option(abi.OPT_PROFILE, 1)
        be.set_option(abi.OPT_JIT, jit)
        return be

    try:
        be = backend(1); variants["a_frame_by_frame"] = (be, FrameByFrame(be, bufs, params_m, types, mats_m, rows, meshes))
        be = backend(2); variants["b_clip_params"] = (be, warp.ClipParamsCall(be, bufs, params_m, types, mats_m, rows))
        be = backend(2); variants["c_clip_lens"] = (be, warp.ClipLensCall(be, bufs, params_m, types, mats_m, rows, meshes=meshes))
        be = backend(2); variants["d_constant_lens_floor"] = (be, warp.ClipParamsCall(be, bufs, params_s, types, mats_s, rows))
        for name, (be, call) in variants.items():          # warm-up: every kernel this form uses is built and loaded
            call()
            be.synchronize()
            be.get_profile_frames(reset=True)
            res[name] = {"us_per_frame": [], "wall_us_per_frame": [], "backend": warp.Backend.last_backend_of(be)}
        for rep in range(a.reps):                           # the variants alternate
            for name, (be, call) in variants.items():
                t0 = time.perf_counter()
                call()
                be.synchronize()
                wall = time.perf_counter() - t0
                ms, launches, covered = be.get_profile_frames(reset=True)
                r = res[name]
                r["us_per_frame"].append(round(1000.0 * ms / max(1, covered), 2))
                r["wall_us_per_frame"].append(round(1e6 * wall / a.frames, 2))
                r["launches"], r["covered"] = launches, covered
                print("rep %d %-22s %8.2f us/frame kernel, %8.2f us/frame wall, %d launches over %d frames (%s)" % (
                    rep, name, r["us_per_frame"][-1], r["wall_us_per_frame"][-1], launches, covered, r["backend"]), flush=True)
        for name in variants:
            v = res[name]["us_per_frame"]
            res[name]["min"], res[name]["max"], res[name]["median"] = min(v), max(v), float(np.median(v))
            print("%-22s kernel us/frame: median %.2f, spread %.2f .. %.2f" % (name, res[name]["median"], min(v), max(v)))
    finally:
        for be in backends:
            be.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
