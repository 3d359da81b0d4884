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
                                                                             [--stab] [--mesh none|shared|per-frame]
--stab gives every frame IBIS/OIS splines (19 control points each, another phase per frame), --mesh a 9 x 9 lens mesh with a focal-plane-distortion block —
one array for the whole clip (uploaded once) or one per frame: route (a) then packs each round's shifts on the host (frame_transform.rs:412-435) and hands them and
the frame's mesh to gfw_undistort_points, route (b) is gfw_zoom_fovs_stab.  Without either the tool runs exactly what it ran before them.
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


def stab_for(k):
    """camera_stab_data[frame k]: a 6000 x 3376 sensor cropped to 5760 x 3240, a few pixels of shift at 4K"""
    pos = np.linspace(-200.0, 3900.0, 19)
    ph = 0.37 * k
    ibis = np.stack([pos, 40.0 * np.sin(pos * 0.004 + ph), -40.0 * np.cos(pos * 0.003 - ph), 100.0 * np.sin(pos * 0.002 + 0.4 + ph)], axis=1)
    ois = np.stack([pos, 15.0 * np.cos(pos * 0.005 - ph), 15.0 * np.sin(pos * 0.006 + ph), np.zeros_like(pos)], axis=1)
    return {"offset": 12.5, "sensor_size": (6000.0, 3376.0), "crop_area": (120.0, 68.0, 5760.0, 3240.0), "pixel_pitch": (3.0, 3.0),
            "width": float(W), "height": float(H), "ibis": ibis, "ois": ois}


def mesh_for(k):
    """a Sony-style mesh block (header, 9 x 9 grid, cubic coefficients per row for x and y, focal-plane-distortion data), f64; k varies the coefficients"""
    n = 9
    m = np.zeros(839, dtype=np.float64)
    o = 9 + n * n * 2 + n * n * 4 * 2
    m[0:9] = (o, n, n, W, H, 0.0, 0.0, W, H)
    base = 9 + n * n * 2
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    for comp, (a, b, c, d) in enumerate(((i * W / 8.0 + 6.0 * np.sin(0.7 * i + 0.3 * j + 0.01 * k), 1.0 + 0.01 * np.cos(i + j), 1e-5 * (i - 4), -1e-9 * (j - 3)),
                                         (j * H / 8.0 + 5.0 * np.cos(0.5 * i - 0.2 * j + 0.01 * k), 0.004 * np.sin(i - j), 2e-6 * (j - 4), 1e-10 * (i - 2)))):
        for jj in range(n):
            rb = base + comp * n * n * 4 + jj * n * 4
            m[rb:rb + n], m[rb + n:rb + 2 * n], m[rb + 2 * n:rb + 3 * n], m[rb + 3 * n:rb + 4 * n] = a[jj], b[jj], c[jj], d[jj]
    m[o] = 1.0
    m[o + 4:o + 20:2] = 0.002 * (np.arange(8) - 3)
    m[o + 5:o + 20:2] = -0.001 * (np.arange(8) - 4)
    return m


def catmull_rom_many(pts, t):
    """CatmullRom::interpolate (gyro_source/splines.rs:22-84) at an array of positions -> [n][3] (zeros where None)"""
    pos, n = pts[:, 0], len(pts)
    lo = np.searchsorted(pos, t, side="left")
    hit = (lo < n) & (pos[np.minimum(lo, n - 1)] == t)
    lower = np.where(hit, lo, lo - 1)
    ok = np.where(hit, lo != n - 1, (lo < n) & (lo != 0)) & (lower + 1 < n) & (lower >= 0)
    lw = np.clip(lower, 0, n - 2)
    a, b = pts[lw, 1:], pts[lw + 1, 1:]
    k = ((t - pos[lw]) / (pos[lw + 1] - pos[lw]))[:, None]
    x = np.where((lw <= 0)[:, None], a * 2.0 - b, pts[np.maximum(lw - 1, 0), 1:])
    y = np.where((lw + 2 >= n)[:, None], b * 2.0 - a, pts[np.minimum(lw + 2, n - 1), 1:])
    v = ((((a * 3.0 - x) - b * 3.0) + y) * 0.5) * k * k * k + ((b - x) * 0.5) * k + a + (((b * 4.0 + a * -5.0 + x + x) - y) * 0.5) * k * k
    return np.where(ok[:, None], v, 0.0)


def shifts_for(stab, pts):
    """at_timestamp_for_points' shifts (frame_transform.rs:412-432) of one round's points (rolling shutter: one per point) -> [n][5] f32"""
    ca, pp = stab["crop_area"], stab["pixel_pitch"]
    sx, sy = W / ca[2] / pp[0], H / ca[3] / pp[1]
    ys = pts[:, 1].astype(np.float64) * ((ca[1] + ca[3]) - ca[1]) / float(H) + ca[1] + stab["offset"]
    s, o = catmull_rom_many(stab["ibis"], ys), catmull_rom_many(stab["ois"], ys)
    return np.stack([s[:, 0] * sx, s[:, 1] * sy, (s[:, 2] / 1000.0) * (np.pi / 180.0), o[:, 0] * sx, o[:, 1] * sy], axis=1).astype(np.float32)


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


def route_a(be, kp, org, smo, nk, timestamps, rect, stabs=None, meshes=None):
    """-> (fovs, seconds inside gfw_undistort_points, calls)"""
    a = f32(f32(H) / f32(W))
    fovs, t_calls, calls = [], 0.0, 0
    frame = 0

    def mapped(ts, pts):
        nonlocal t_calls, calls
        rot = rotations_for(org, smo, nk, ts, pts)
        sh = shifts_for(stabs[frame], pts) if stabs is not None else None
        mesh = meshes[frame] if meshes is not None else None
        t0 = time.perf_counter()
        out = be.undistort_points(kp, rot, points=pts, shifts=sh, index_mode=abi.POINT_INDEX_PER_POINT, mesh=mesh)
        t_calls += time.perf_counter() - t0
        calls += 1
        return out
    for frame, ts in enumerate(timestamps):
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
    ap.add_argument("--stab", action="store_true", help="every frame has IBIS/OIS splines: per-point shifts")
    ap.add_argument("--mesh", choices=("none", "shared", "per-frame"), default="none", help="lens mesh + focal-plane distortion: one array for the clip, or one per frame")
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
    stabs = [stab_for(k) for k in range(n)] if args.stab else None
    meshes = None
    if args.mesh == "shared":
        meshes = [mesh_for(0)] * n
    elif args.mesh == "per-frame":
        meshes = [mesh_for(k) for k in range(n)]
    with_data = stabs is not None or meshes is not None

    def search_all(**kw):
        if with_data:
            return be.zoom_fovs_stab(kp, search, frames, stabs=stabs, meshes=meshes, **kw)
        return be.zoom_fovs(kp, search, frames, **kw)
    result = {"frames": n, "stab": bool(args.stab), "mesh": args.mesh, "frames_a": min(args.frames_a, n), "lens_correction_amount": args.lca, "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        be.set_quaternion_tracks(org, smo)
        search_all()                                                          # warm-up: allocations, code object load
        route_a(be, kp, org, smo, nk, timestamps[:4], rect, stabs, meshes)
        d_out = torch.zeros(n, dtype=torch.float64, device=dev)
        for rep in range(args.reps):
            na = min(args.frames_a, n)
            t0 = time.perf_counter()
            fa, t_calls, calls = route_a(be, kp, org, smo, nk, timestamps[:na], rect, stabs, meshes)
            wall_a = time.perf_counter() - t0
            t0 = time.perf_counter()
            fb = search_all()
            wall_b = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            search_all(out_ptr=d_out.data_ptr())
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
    print("%s for all %d frames takes less wall time than the gfw_undistort_points calls of route (a) alone, extrapolated: %s" % ("gfw_zoom_fovs_stab" if with_data else "gfw_zoom_fovs", n, ok))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
