#!/usr/bin/env python3
"""A 4K 16-bit 4:2:2 dynamic-zoom clip (per-frame fov, moving zoom centre — what FrameTransform::at_timestamp hands a render with adaptive zoom on) three ways,
kernel time per frame from gfw_get_profile_frames:
  (a) gfw_undistort_frame frame by frame (each frame's own params; GFW_OPT_JIT = 1, the default: the zoom centre moves every frame, so the constant-parameter
      specialisation never gets its three frames and the clip stays on the ahead-of-time kernels),
  (b) gfw_undistort_clip_params (the per-frame flavour of the specialised kernel, shared launches),
  (c) gfw_undistort_clip with one constant params block (the pre-existing multi-frame path; not the same pixels — the speed it is measured against).
HIP_DEVICE buffers, packed device tables, GFW_OPT_JIT = 2 for (b) and (c).  usage: clip_params_bench.py [--frames N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402

W, H = 3840, 2160


def frames_of(n):
    return [S.SyntheticFrame("YUV422P16LE", W, H, seed=0xC1 + f, timestamp_ms=1000.0 + 33.3 * f, fov=1.0 + 0.02 * (f % 12), pixels=False,
                             base_overrides={"translation2d": (-24.0 + 4.0 * (f % 12), 13.5 - 2.25 * (f % 12))}) for f in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    frames = frames_of(a.frames)
    d_src = [fr.device_planes(dev) for fr in frames]
    d_dst = [fr.device_outputs(dev) for fr in frames]
    d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [[pl["params"] for pl in fr.planes] for fr in frames]
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(), d_dst[j][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
    rows = frames[0].matrices.shape[0]
    mats = [m.data_ptr() for m in d_mat]
    be = warp.Backend(params[0][0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    res = {"clip": "4K YUV422P16LE, fisheye, bilinear, fov 1.00-1.22, moving zoom centre", "frames": a.frames, "reps": a.reps}
    try:
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        be.set_option(abi.OPT_PROFILE, 1)
        calls = {
            "a_frame_by_frame": [warp.FrameCall(be, bufs[j], params[j], types, mats[j], rows) for j in range(a.frames)],
            "b_clip_params": [warp.ClipParamsCall(be, bufs, params, types, mats, rows)],
            "c_clip_constant": [warp.ClipCall(be, bufs, params[0], types, mats, rows)],
        }
        for name, cs in calls.items():
            be.set_option(abi.OPT_JIT, 1 if name.startswith("a_") else 2)
            for c in cs:                              # warm-up: the specialised kernel of this form is built and loaded
                c()
            be.synchronize()
            be.get_profile_frames(reset=True)
            for _ in range(a.reps):
                for c in cs:
                    c()
            be.synchronize()
            ms, launches, covered = be.get_profile_frames(reset=True)
            res[name] = {"us_per_frame": round(1000.0 * ms / max(1, covered), 2), "launches": launches, "frames": covered, "backend": warp.last_backend()}
            print(name, json.dumps(res[name]), flush=True)
    finally:
        be.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
