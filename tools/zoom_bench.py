#!/usr/bin/env python3
"""The adaptive-zoom FOV search (FovIterative::find_fov per frame) over the 10 000-frame C5 clip's tracks — 4K source, 16 ms readout, the tracks bench.py --c5
uses — two ways:
  (a) through the ABI without gfw_zoom_fovs: per frame and round, the rotations of the round's points on the host (f64 slerp over the tracks, numpy-vectorised
      over the points), one synchronous gfw_undistort_points call, the fold on the host, the next points chosen from it.  Run for the first --frames-a frames and
      extrapolated to the clip; the time spent INSIDE the gfw_undistort_points calls (upload, launch, synchronise, download) is reported on its own, so that the
      host-side Python of this tool can be told from what any caller of that ABI pays;
  (b) gfw_zoom_fovs for all frames in one call (host outputs: wall time includes the descriptor upload and the result download), and the kernel time alone from
      hipEvents around an asynchronous call with device outputs.
Prints both, frames per second, and how far the two results differ.  usage: zoom_bench.py [--frames N] [--frames-a M] [--reps R] [--lca A] [--out FILE]
(GFW_LIBRARY selects an A/B build of the library.)"""
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

W, H, READOUT = 3840, 2160, 16.0
f32 = np.float32


def quat_at_many(ts_us, quats, t_ms):
    """GyroSource::quat_at_timestamp over an array of times (no sync offsets): nalgebra's slerp, vectorised"""
    lookup = np.clip(np.round(t_ms * 1000.0).astype(np.int64), ts_us[0], ts_us[-1])
    i = np.searchsorted(ts_us, lookup, side="right") - 1
    j = np.minimum(i + 1, len(ts_us) - 1)
    a, b = quats[i], quats[j].copy()
    span = np.maximum(ts_us[j] - ts_us[i], 1)
    t = ((lookup - ts_us[i]) / span)[:, None]
    c = np.sum(a * b, axis=1, keepdims=True)
    b = np.where(c < 0.0, -b, b)
    c = np.abs(c)
    hang = np.arccos(np.minimum(c, 1.0))
    s = np.sqrt(np.maximum(1.0 - c * c, 0.0))
    ok = (s > 0.0) & (c < 1.0)
    sd = np.where(ok, s, 1.0)
    out = a * (np.sin((1.0 - t) * hang) / sd) + b * (np.sin(t * hang) / sd)
    return np.where(ok, out, a)


def qmul_many(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def rotations_for(org, smo, nk, ts, pts):
    """at_timestamp_for_points (frame_transform.rs:376-410) for one frame's points -> [n][9] f32"""
    start = ts - READOUT / 2.0
    qt = start + (READOUT / H) * pts[:, 1].astype(np.float64)
    q1 = quat_at_many(org[0], org[1], np.array([ts]))[0]
    q1 = np.array([q1[0], -q1[1], -q1[2], -q1[3]]) / np.dot(q1, q1)
    pre = qmul_many(quat_at_many(smo[0], smo[1], np.array([ts]))[0], q1)
    q = qmul_many(pre[None, :], quat_at_many(org[0], org[1], qt))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    r = np.stack([1 - 2 * (y * y + z * z), -2 * (x * y - z * w), -2 * (x * z + y * w),
                  -2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  -2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)     # with the four sign flips
    return (nk[None, :, :] @ r).reshape(-1, 9).astype(np.float32)


def rect_points():
    w, h = f32(W), f32(H)
    ws, hs = f32(w / f32(30)), f32(h / f32(30))
    p = [(f32(i) * ws, f32(0)) for i in range(30)] + [(w, f32(i) * hs) for i in range(30)] + \
        [(f32(30 - i) * ws, h) for i in range(30)] + [(f32(0), f32(30 - i) * hs) for i in range(30)]
    return np.array(p, dtype=np.float32)


def fold(poly, m, a):
    idx = None
    cx, cy = f32(W / 2), f32(H / 2)
    for i in range(len(poly)):
        ap0, ap1 = abs(f32(poly[i, 0] - cx)), abs(f32(poly[i, 1] - cy))
        if ap0 < m[0] and ap1 < m[1]:
            m = (f32(ap1 / a), ap1) if ap1 > f32(ap0 * a) else (ap0, f32(ap0 * a))
            idx = i
    return idx, m


def route_a(be, kp, org, smo, nk, timestamps, rect):
    """-> (fovs, seconds inside gfw_undistort_points, calls)"""
    a = f32(f32(H) / f32(W))
    fovs, t_calls, calls = [], 0.0, 0

    def mapped(ts, pts):
        nonlocal t_calls, calls
        rot = rotations_for(org, smo, nk, ts, pts)
        t0 = time.perf_counter()
        out = be.undistort_points(kp, rot, points=pts, index_mode=abi.POINT_INDEX_PER_POINT)
        t_calls += time.perf_counter() - t0
        calls += 1
        return out
    for ts in timestamps:
        poly = mapped(ts, rect)
        idx, m = None, (f32(1000000.0), f32(f32(1000000.0) * a))
        for _ in range(1, 5):
            idx, m = fold(poly, m, a)
            if idx is None:
                break
            rel = rect[[15 if idx == 0 else idx - 1, idx, (idx + 1) % 120]]
            i = np.arange(63)
            i1, fr = i // 31, (i % 31).astype(np.float32) / f32(31)
            i2 = np.minimum(i1 + 1, 2)
            pts = (rel[i1] + fr[:, None] * (rel[i2] - rel[i1])).astype(np.float32)
            poly = mapped(ts, pts)
            idx, m = fold(poly, m, a)
        fovs.append(float(f32(f32(m[0] * f32(2)) / f32(W))))
    return np.array(fovs), t_calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--frames-a", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lca", type=float, default=1.0, help="lens_correction_amount of every frame (< 1: the Newton inverse of the blend per point)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.frames
    timestamps = [1000.0 + 33.3 * f for f in range(n)]
    t_end = timestamps[-1] + 200.0
    org = S.sampled_track_fast(11, 0.0, t_end, 500.0)
    smo = S.sampled_track_fast(12, 0.0, t_end, 100.0, scale=0.25)
    lens = S.gopro_style_lens(W, H)
    nk = S.new_k(lens, 1.0, W, H)
    kp = S.base_kernel_params(lens, 1.0, 1, lens_correction_amount=args.lca)
    kp.width, kp.height, kp.output_width, kp.output_height = W, H, W, H
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1, lens=lens)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    search = abi.ZoomSearch(width=W, height=H, org_output_width=W, org_output_height=H, fov_algorithm_margin=0.0, horizontal_readout=0)
    frames = (abi.ZoomFrame * n)()
    for k, ts in enumerate(timestamps):
        f = frames[k]
        f.timestamp_ms, f.frame_readout_time_ms, f.fov, f.lens_correction_amount = ts, READOUT, 1.0, args.lca
        for i, v in enumerate(nk.reshape(9)):
            f.new_k[i] = v
    rect = rect_points()
    result = {"frames": n, "frames_a": min(args.frames_a, n), "lens_correction_amount": args.lca, "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        be.set_quaternion_tracks(org, smo)
        be.zoom_fovs(kp, search, frames)                                      # warm-up: allocations, code object load
        route_a(be, kp, org, smo, nk, timestamps[:4], rect)
        d_out = torch.zeros(n, dtype=torch.float64, device=dev)
        for rep in range(args.reps):
            na = min(args.frames_a, n)
            t0 = time.perf_counter()
            fa, t_calls, calls = route_a(be, kp, org, smo, nk, timestamps[:na], rect)
            wall_a = time.perf_counter() - t0
            t0 = time.perf_counter()
            fb = be.zoom_fovs(kp, search, frames)
            wall_b = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            be.zoom_fovs(kp, search, frames, out_ptr=d_out.data_ptr())
            e1.record(stream)
            e1.synchronize()
            kernel_ms = e0.elapsed_time(e1)
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            run = {"a_wall_s": wall_a, "a_inside_calls_s": t_calls, "a_calls": calls, "a_extrapolated_s": wall_a * n / na, "a_calls_extrapolated_s": t_calls * n / na,
                   "b_wall_s": wall_b, "b_stream_ms": kernel_ms, "b_frames_per_s": n / wall_b, "max_rel_difference": float(np.max(np.abs(fa - fb[:na]) / fb[:na])),
                   "device_matches_host_output": bool(np.array_equal(d_out.cpu().numpy(), fb)), "fov_minimal_range": [float(fb.min()), float(fb.max())]}
            result["runs"].append(run)
            print("run %d: (a) %d frames %.3f s (%.3f s inside %d gfw_undistort_points calls) -> %.1f s (%.1f s) for %d frames, %.0f frames/s | "
                  "(b) %d frames %.4f s wall, %.3f ms on the stream (copy in + launch), %.0f frames/s, fov_minimal %.4f .. %.4f | results differ by %.2g relative"
                  % (rep, na, wall_a, t_calls, calls, run["a_extrapolated_s"], run["a_calls_extrapolated_s"], n, na / wall_a,
                     n, wall_b, kernel_ms, run["b_frames_per_s"], fb.min(), fb.max(), run["max_rel_difference"]), flush=True)
    finally:
        be.close()
    ok = all(r["b_wall_s"] < r["a_calls_extrapolated_s"] for r in result["runs"])
    print("gfw_zoom_fovs for all %d frames takes less wall time than the gfw_undistort_points calls of route (a) alone, extrapolated: %s" % (n, ok))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
