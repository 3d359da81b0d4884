#!/usr/bin/env python3
"""Pyramidal Lucas-Kanade optical flow (optical_flow/opencv_pyrlk.rs) at the size of a sync: 5 sync points x 46 analysed frames = 225 frame pairs of 200 features at
1280 x 720, the frames resident in device memory — gfw_flow_pyrlk in one call:
wall time with host outputs, and time on the stream (events around an asynchronous call with device outputs).
The frames are crops of one analytic texture (a sum of plane waves) shifted by whole pixels from frame to frame, 2 .. 7 px a pair.
The first `--check` pairs are compared with the numpy statement of the tests (tests/_flowstmt.py) to the bit.  Nothing is timed against the reference, which runs
OpenCV per frame on a thread pool and cannot be built here.
usage: flow_bench.py [--groups N] [--frames N] [--features N] [--width W] [--height H] [--reps R] [--check N] [--out FILE]   (GFW_LIBRARY selects an A/B build.)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402
import _flowstmt as FS  # noqa: E402

ORDER = ("next", "status", "iters", "grid_points", "grid_counts", "pair_first", "points_a", "points_b")


def clip(groups, per_group, width, height, seed=1):
    """-> (frames u8 [n][height][width], pairs, shifts): frame k of a group is the texture cropped at the group's running whole-pixel offset"""
    g = np.random.default_rng(seed)
    margin = 8 * per_group
    ys, xs = np.mgrid[0:height + margin, 0:width + margin].astype(np.float32)
    tex = np.full(xs.shape, 128.0, dtype=np.float32)
    lam = 6.0 * 10.0 ** g.uniform(0.0, 1.0, 24)
    amp = lam ** 0.5 * g.uniform(0.5, 1.0, 24)
    amp *= 45.0 / np.sqrt(0.5 * (amp ** 2).sum())
    for l, a, t, p in zip(lam, amp, g.uniform(0.0, 2.0 * np.pi, 24), g.uniform(0.0, 2.0 * np.pi, 24)):
        tex += np.float32(a) * np.cos(xs * np.float32(2.0 * np.pi / l * np.cos(t)) + ys * np.float32(2.0 * np.pi / l * np.sin(t)) + np.float32(p))
    tex = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
    frames, pairs, shifts = [], [], []
    for _ in range(groups):
        ox = oy = 0
        for k in range(per_group):
            if k:
                dx, dy = int(g.integers(2, 8)), int(g.integers(0, 4))
                ox, oy = ox + dx, oy + dy
                pairs.append((len(frames) - 1, len(frames)))
                shifts.append((-dx, -dy))
            frames.append(tex[oy:oy + height, ox:ox + width])
    return np.ascontiguousarray(np.stack(frames)), pairs, shifts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--frames", type=int, default=46)
    ap.add_argument("--features", type=int, default=200)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    frames, pairs, shifts = clip(args.groups, args.frames, args.width, args.height)
    g = np.random.default_rng(2)
    feats = [np.stack([g.uniform(16.0, args.width - 16.0, args.features), g.uniform(16.0, args.height - 16.0, args.features)], axis=1).astype(np.float32) for _ in frames]
    raw = len(pairs) * args.features
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"pairs": len(pairs), "features": args.features, "size": [args.width, args.height], "frames": len(frames), "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        d_frames = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize(dev)
        be.flow_pyrlk(d_frames.data_ptr(), args.width, pairs, feats, shape=frames.shape)       # warm-up: allocations, code object load
        t0 = time.perf_counter()
        want = FS.flow_pyrlk(frames, pairs[:args.check], feats)
        stmt_s = (time.perf_counter() - t0) / max(args.check, 1)
        k = args.check * args.features
        outs = {"next": torch.zeros((raw, 2), dtype=torch.float32, device=dev), "status": torch.zeros(raw, dtype=torch.uint8, device=dev), "iters": None, "grid_points": None,
                "grid_counts": None, "pair_first": torch.zeros(len(pairs) + 1, dtype=torch.int32, device=dev), "points_a": torch.zeros((raw, 2), dtype=torch.float32, device=dev),
                "points_b": torch.zeros((raw, 2), dtype=torch.float32, device=dev)}
        for rep in range(args.reps):
            t0 = time.perf_counter()
            got = be.flow_pyrlk(d_frames.data_ptr(), args.width, pairs, feats, iters=True, shape=frames.shape)
            wall = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            be.flow_pyrlk(d_frames.data_ptr(), args.width, pairs, feats, out_ptrs=tuple(None if outs[n] is None else outs[n].data_ptr() for n in ORDER), shape=frames.shape)
            e1.record(stream)
            e1.synchronize()
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            tracked = got["status"] == 1
            flow = got["next"] - np.concatenate([feats[a] for a, _ in pairs])
            err = np.linalg.norm(flow - np.repeat(np.array(shifts, dtype=np.float32), args.features, axis=0), axis=1)
            run = {"wall_s": wall, "stream_ms": e0.elapsed_time(e1), "statement_s_per_pair": stmt_s,
                   "device_equals_statement": got["next"][:k].tobytes() == want["next"].tobytes() and got["status"][:k].tobytes() == want["status"].tobytes()
                   and got["iters"][:k].tobytes() == want["iters"].tobytes(),
                   "device_output_equals_host_output": outs["next"].cpu().numpy().tobytes() == got["next"].tobytes() and outs["pair_first"].cpu().numpy().tobytes() == got["pair_first"].tobytes(),
                   "tracked_share": float(tracked.mean()), "kept": int(got["pair_first"][-1]), "median_error_px": float(np.median(err[tracked])),
                   "mean_updates_per_level": [float(v) for v in np.where(got["iters"] < 0, 0, got["iters"])[tracked].mean(axis=0)]}
            result["runs"].append(run)
            print("run %d: gfw_flow_pyrlk of %d pairs x %d features at %d x %d: %.3f ms wall with host outputs, %.3f ms on the stream | the numpy statement %.2f s a pair | "
                  "device = statement on %d pairs: %s | tracked %.3f, median error %.4f px, updates a level %s" %
                  (rep, len(pairs), args.features, args.width, args.height, wall * 1e3, run["stream_ms"], stmt_s, args.check, run["device_equals_statement"],
                   run["tracked_share"], run["median_error_px"], ["%.1f" % v for v in run["mean_updates_per_level"]]), flush=True)
    finally:
        be.close()
    ok = all(r["device_equals_statement"] and r["device_output_equals_host_output"] for r in result["runs"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
