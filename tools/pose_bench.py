#!/usr/bin/env python3
"""Almeida pose estimation (estimate_pose/almeida.rs) at the size of a sync: 5 sync points x about 45 frame pairs = 225 pairs of 200 matched points, 200 rounds and
1000 samples (the reference's defaults), the library's draws — gfw_pose_almeida in one call:
  (a) with host outputs (wall time: staging, upload, four launches, download);
  (b) the time on the stream alone, from events around an asynchronous call with device outputs.
The first `--check` pairs are compared with the numpy statement of the tests (tests/_posestmt.py) to the bit.  Nothing is timed against the reference, which runs
its rounds under rayon on all host cores and cannot be built here; the statement's time per pair is context, not a pass mark.
usage: pose_bench.py [--pairs N] [--points N] [--rounds N] [--reps R] [--check N] [--out FILE]   (GFW_LIBRARY selects an A/B build of the library.)"""
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
import _posecase as PC  # noqa: E402
import _posestmt as PS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=225)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    cam = PS.Camera(PC.pinhole_clip(), (960, 540), num_iters=args.rounds)
    g = np.random.default_rng(1)
    pairs = [PC.plant_f64(cam, args.points, tuple(g.uniform(-3.0, 3.0, 3)), 0.3, 100 + k)[:2] for k in range(args.pairs)]
    triples, samples = warp.pose_draws(1, [args.points] * args.pairs, args.rounds, cam.num_samples)
    cfg = PC.cfg_of(cam)
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"pairs": args.pairs, "points": args.points, "rounds": args.rounds, "samples": cam.num_samples, "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        be.pose_almeida(cam.kp, cfg, pairs, triples, samples)                 # warm-up: allocations, code object load
        t0 = time.perf_counter()
        want = PS.estimate(cam, pairs[:args.check], triples[:args.check], samples[:args.check])
        stmt_s = (time.perf_counter() - t0) / max(args.check, 1)
        outs = (torch.zeros((args.pairs, 4), dtype=torch.float32, device=dev), torch.zeros((args.pairs, 9), dtype=torch.float64, device=dev),
                torch.zeros((args.pairs, 2), dtype=torch.int32, device=dev))
        for rep in range(args.reps):
            t0 = time.perf_counter()
            quats, rot, best = be.pose_almeida(cam.kp, cfg, pairs, triples, samples)
            wall = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            be.pose_almeida(cam.kp, cfg, pairs, triples, samples, out_ptrs=tuple(o.data_ptr() for o in outs) + (None, None))
            e1.record(stream)
            e1.synchronize()
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            k = args.check
            run = {"wall_s": wall, "stream_ms": e0.elapsed_time(e1), "statement_s_per_pair": stmt_s,
                   "device_equals_statement": quats[:k].tobytes() == want[0].tobytes() and rot[:k].tobytes() == want[1].tobytes() and best[:k].tobytes() == want[2].tobytes(),
                   "device_output_equals_host_output": outs[0].cpu().numpy().tobytes() == quats.tobytes() and outs[1].cpu().numpy().tobytes() == rot.tobytes(),
                   "median_inliers": float(np.median(best[:, 0]))}
            result["runs"].append(run)
            print("run %d: gfw_pose_almeida of %d pairs x %d points x %d rounds: %.3f ms wall with host outputs, %.3f ms on the stream | the numpy statement %.2f s a pair | "
                  "device = statement on %d pairs: %s" % (rep, args.pairs, args.points, args.rounds, wall * 1e3, run["stream_ms"], stmt_s, k, run["device_equals_statement"]), flush=True)
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
