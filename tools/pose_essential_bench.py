#!/usr/bin/env python3
"""Essential-matrix pose estimation (pose methods 0 and 2) at the size of a sync: 5 sync points x about 45 frame pairs = 225 pairs of 200 matched points, 200 rounds,
the library's draws — gfw_pose_essential in one call:
  (a) with host outputs (wall time: staging, upload, four launches, download);
  (b) the time on the stream alone, from events around an asynchronous call with device outputs.
The first `--check` pairs are compared with the numpy statement of the tests (tests/_posessstmt.py) to the bit.  gfw_pose_almeida on the SAME pairs (200 rounds, its
default 1000 samples) is timed beside it for scale: another algorithm with another answer, not a baseline.  A record, not a pass mark: there is no parent-commit
figure, and nothing is timed against the reference, whose solvers for these methods are not in its tree.
usage: pose_essential_bench.py [--pairs N] [--points N] [--rounds N] [--reps R] [--check N] [--out FILE]   (GFW_LIBRARY selects an A/B build of the library.)"""
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
import _posesscase as EC  # noqa: E402
import _posessstmt as ES  # noqa: E402
import _posestmt as PS  # noqa: E402


def timed(be, dev, call_host, call_device):
    """-> (host-output result, wall seconds, stream milliseconds)"""
    import torch
    t0 = time.perf_counter()
    got = call_host()
    wall = time.perf_counter() - t0
    stream = torch.cuda.current_stream(dev)
    be.set_stream(stream.cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call_device()
    e1.record(stream)
    e1.synchronize()
    be.set_option(abi.OPT_SYNCHRONOUS, 1)
    return got, wall, e0.elapsed_time(e1)


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
    cam = ES.Camera(EC.pinhole_clip(), (1920, 1080), num_iters=args.rounds)
    pairs = [EC.plant_scene(cam, args.points, 0.2, 100 + k)[:2] for k in range(args.pairs)]
    octets = warp.pose_draws_k(1, [args.points] * args.pairs, args.rounds, 8)
    cfg = EC.cfg_of(cam)
    acam = PS.Camera(EC.pinhole_clip(), (1920, 1080), num_iters=args.rounds)
    triples, samples = warp.pose_draws(1, [args.points] * args.pairs, args.rounds, acam.num_samples)
    acfg = PC.cfg_of(acam)
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"pairs": args.pairs, "points": args.points, "rounds": args.rounds, "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        be.pose_essential(cam.kp, cfg, pairs, octets)                       # warm-up: allocations, code object load
        be.pose_almeida(acam.kp, acfg, pairs, triples, samples)
        t0 = time.perf_counter()
        want = ES.estimate(cam, pairs[:args.check], octets[:args.check])
        stmt_s = (time.perf_counter() - t0) / max(args.check, 1)
        n = args.pairs
        outs = (torch.zeros((n, 4), dtype=torch.float32, device=dev), torch.zeros((n, 9), dtype=torch.float64, device=dev),
                torch.zeros((n, 9), dtype=torch.float64, device=dev), torch.zeros((n, 4), dtype=torch.int32, device=dev))
        aouts = (torch.zeros((n, 4), dtype=torch.float32, device=dev), torch.zeros((n, 9), dtype=torch.float64, device=dev), torch.zeros((n, 2), dtype=torch.int32, device=dev))
        for rep in range(args.reps):
            (quats, rot, ess, best), wall, stream_ms = timed(
                be, dev, lambda: be.pose_essential(cam.kp, cfg, pairs, octets),
                lambda: be.pose_essential(cam.kp, cfg, pairs, octets, out_ptrs=tuple(o.data_ptr() for o in outs) + (None, None)))
            _, awall, astream_ms = timed(
                be, dev, lambda: be.pose_almeida(acam.kp, acfg, pairs, triples, samples),
                lambda: be.pose_almeida(acam.kp, acfg, pairs, triples, samples, out_ptrs=tuple(o.data_ptr() for o in aouts) + (None, None)))
            k = args.check
            same = all(g[:k].tobytes() == w.tobytes() for g, w in zip((quats, rot, ess, best), want[:4]))
            dev_same = all(o.cpu().numpy().reshape(g.shape).tobytes() == g.tobytes() for o, g in zip(outs, (quats, rot, ess, best)))
            run = {"wall_s": wall, "stream_ms": stream_ms, "almeida_wall_s": awall, "almeida_stream_ms": astream_ms, "statement_s_per_pair": stmt_s,
                   "device_equals_statement": same, "device_output_equals_host_output": dev_same,
                   "median_inliers": float(np.median(best[:, 0])), "found": int(best[:, 3].sum())}
            result["runs"].append(run)
            print("run %d: gfw_pose_essential of %d pairs x %d points x %d rounds: %.3f ms wall with host outputs, %.3f ms on the stream | gfw_pose_almeida on the same "
                  "pairs: %.3f ms wall, %.3f ms on the stream | the numpy statement %.2f s a pair | device = statement on %d pairs: %s | found %d, median inliers %.0f"
                  % (rep, args.pairs, args.points, args.rounds, wall * 1e3, stream_ms, awall * 1e3, astream_ms, stmt_s, k, same, run["found"], run["median_inliers"]), flush=True)
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
