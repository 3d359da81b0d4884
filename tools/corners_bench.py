#!/usr/bin/env python3
"""Shi-Tomasi corner detection (optical_flow/opencv_pyrlk.rs:25-42) at the size of a sync: the first 226 frames of tools/flow_bench.py's clip (1280 x 720, crops of
one analytic texture), resident in device memory, with the reference's parameters (200 corners, quality 0.01, distance 10) — gfw_corners_shi_tomasi in one call:
wall time with host outputs, and time on the stream (events around an asynchronous call with device outputs).
The first `--check` frames are compared with the numpy statement of the tests (tests/_cornerstmt.py) to the bit; their candidate counts (the positive local maxima
the device lists, and those above the threshold) and the rounds the pick takes come from the statement.  Nothing is timed against the reference, which runs OpenCV
per frame on a thread pool and cannot be built here.  Per-launch times: run this under a kernel trace, in a run of its own.
usage: corners_bench.py [--frames N] [--width W] [--height H] [--reps R] [--check N] [--max-workspace-mb M] [--out FILE]   (GFW_LIBRARY selects an A/B build.)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402
import _cornerstmt as CS  # noqa: E402
import flow_bench  # noqa: E402

ORDER = ("corners", "scores", "counts", "feat_first", "features")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=226)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--max-workspace-mb", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    per_group = 46
    frames = flow_bench.clip((args.frames + per_group - 1) // per_group, per_group, args.width, args.height)[0][:args.frames]
    n, m = len(frames), CS.MAX_CORNERS
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    list_bytes = (args.width - 2) * (args.height - 2) * 8
    per_batch = min(n, ((args.max_workspace_mb or abi.CORNERS_WORKSPACE_MB) << 20) // list_bytes)
    result = {"frames": n, "size": [args.width, args.height], "max_corners": m, "quality": CS.QUALITY, "min_distance": CS.MIN_DISTANCE, "library": os.environ.get("GFW_LIBRARY", ""),
              "batches": (n + per_batch - 1) // per_batch, "frames_per_batch": per_batch, "launches": 2 * ((n + per_batch - 1) // per_batch) + 2, "checked": [], "runs": []}
    try:
        d_frames = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize(dev)
        be.corners_shi_tomasi(d_frames.data_ptr(), args.width, max_workspace_mb=args.max_workspace_mb, shape=frames.shape)       # warm-up: allocations, code object load
        t0 = time.perf_counter()
        want = []
        for f in range(min(args.check, n)):
            st, rounds = {}, {}
            want.append(CS.detect(frames[f], stats=st))
            e = CS.min_eigen(frames[f])
            listed = CS.keys(e, CS.candidates_raw(e, np.float32(0.0)))
            CS.pick_rounds(listed, args.width, m, CS.MIN_DISTANCE, st["threshold"], rounds)
            result["checked"].append({"frame": f, "listed": int(len(listed)), "above_threshold": int(st["candidates"]), "rounds": int(rounds["rounds"]), "corners": int(len(want[-1][0]))})
        stmt_s = (time.perf_counter() - t0) / max(len(want), 1)
        outs = {"corners": torch.zeros((n, m, 2), dtype=torch.float32, device=dev), "scores": torch.zeros((n, m), dtype=torch.float32, device=dev),
                "counts": torch.zeros(n, dtype=torch.int32, device=dev), "feat_first": torch.zeros(n + 1, dtype=torch.int32, device=dev),
                "features": torch.zeros((n * m, 2), dtype=torch.float32, device=dev)}
        for rep in range(args.reps):
            t0 = time.perf_counter()
            got = be.corners_shi_tomasi(d_frames.data_ptr(), args.width, scores=True, max_workspace_mb=args.max_workspace_mb, shape=frames.shape)
            wall = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            be.corners_shi_tomasi(d_frames.data_ptr(), args.width, max_workspace_mb=args.max_workspace_mb, out_ptrs=tuple(outs[k].data_ptr() for k in ORDER), shape=frames.shape)
            e1.record(stream)
            e1.synchronize()
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            same = all(got["counts"][f] == len(c) and got["corners"][f, :len(c)].tobytes() == c.tobytes() and got["scores"][f, :len(c)].tobytes() == s.tobytes() for f, (c, s) in enumerate(want))
            run = {"wall_s": wall, "stream_ms": e0.elapsed_time(e1), "statement_s_per_frame": stmt_s, "device_equals_statement": bool(same),
                   "device_output_equals_host_output": outs["corners"].cpu().numpy().tobytes() == got["corners"].tobytes() and outs["feat_first"].cpu().numpy().tobytes() == got["feat_first"].tobytes(),
                   "corners_min": int(got["counts"].min()), "corners_max": int(got["counts"].max())}
            result["runs"].append(run)
            print("run %d: gfw_corners_shi_tomasi of %d frames at %d x %d (%d batches, %d launches): %.3f ms wall with host outputs, %.3f ms on the stream | the numpy statement %.2f s a frame | "
                  "device = statement on %d frames: %s | corners a frame %d .. %d" %
                  (rep, n, args.width, args.height, result["batches"], result["launches"], wall * 1e3, run["stream_ms"], stmt_s, len(want), same, run["corners_min"], run["corners_max"]), flush=True)
        for c in result["checked"]:
            print("frame %(frame)d: %(listed)d positive local maxima listed, %(above_threshold)d above the threshold, %(rounds)d rounds, %(corners)d corners" % c)
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
