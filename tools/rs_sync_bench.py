#!/usr/bin/env python3
"""The rs-sync offset search (offset method 2) at the size of a sync: 5 ranges x 45 frame pairs x 300 matched points, radius 3000 ms at 3 ms steps (2001 + 3 x 17
candidates a range), 4 rounds, a 1 kHz quaternion track of 20 s — gfw_sync_rs_search in one call:
  (a) with host outputs (wall time: staging, upload, 1 + 2 x rounds launches, download);
  (b) the time on the stream alone, from events around an asynchronous call with device outputs.
Beside it a single-threaded C++ loop of the same arithmetic (tools/rs_sync_cpu.cpp, built here with the host pass of hipcc) over `--cpu-candidates` candidates of
every range, its range costs compared with gfw_sync_rs_costs' to the bit, and its time scaled to the search's candidate count for scale.  A record, not a pass mark:
there is no parent-commit figure, and nothing is timed against the reference, whose solver is not in its tree.
usage: rs_sync_bench.py [--ranges N] [--pairs N] [--points N] [--radius-ms R] [--reps R] [--cpu-candidates N] [--out FILE]   (GFW_LIBRARY selects an A/B build.)"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402
import _posesscase as EC  # noqa: E402
import _posessstmt as ES  # noqa: E402
import _rssynccase as RC  # noqa: E402
import _rssyncstmt as RS  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DELAY_S, READOUT_MS, TRACK_S = 0.0073, 12.0, 20.0


def cpu_loop(tmp, cam, cfg, track, ranges, cands):
    """-> (seconds, costs [n_ranges][n_cand]) of tools/rs_sync_cpu.cpp over the statement's prepared points"""
    exe = os.path.join(tmp, "rs_sync_cpu")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off",
                           os.path.join(ROOT, "tools", "rs_sync_cpu.cpp"), "-o", exe])
    prepared = [RS.prepare(cam, cfg, p[:2], p[2], p[3]) for r in ranges for p in r]
    first = np.zeros(len(prepared) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(p[1]) for p in prepared])
    rf = np.zeros(len(ranges) + 1, dtype=np.int32)
    rf[1:] = np.cumsum([len(r) for r in ranges])
    side = lambda k: np.concatenate([np.concatenate([p[2 * k], p[2 * k + 1][:, None]], axis=1) for p in prepared])
    dump = os.path.join(tmp, "rs_sync_cpu.bin")
    with open(dump, "wb") as f:
        f.write(np.array([len(track[0]), len(ranges), len(prepared), first[-1], len(cands), cfg.hypotheses, cfg.refits, cfg.sweeps], dtype=np.int32).tobytes())
        f.write(np.array([cfg.loss_scale]).tobytes())
        f.write(RS.track_seconds(track[0]).tobytes() + np.ascontiguousarray(track[1], dtype=np.float64).tobytes() + rf.tobytes() + first.tobytes())
        f.write(np.ascontiguousarray(side(0)).tobytes() + np.ascontiguousarray(side(1)).tobytes() + np.asarray(cands, dtype=np.float64).tobytes())
    out = subprocess.run([exe, dump], capture_output=True, text=True, check=True).stdout.split()
    return float(out[0]), np.array([float.fromhex(v) for v in out[1:]]).reshape(len(ranges), len(cands))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranges", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=45)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--radius-ms", type=float, default=3000.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-candidates", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    cam = ES.Camera(EC.pinhole_clip(), RC.FLOW)
    cfg = RS.Cfg(readout_ms=READOUT_MS)
    track = RC.track(1000.0, seconds=TRACK_S)
    v = RC.unit((1.0, 0.4, 0.2), 0.5)
    ranges = [RC.plant_range(cam, [args.points] * args.pairs, DELAY_S, READOUT_MS, v, 1000 * r, 0.3, start_s=4.0 + 3.0 * r) for r in range(args.ranges)]
    c = RC.cfg_of(cam, cfg)
    radius_s = args.radius_ms / 1000.0
    total = warp.sync_rs_candidates(radius_s, c.step_s, c.rounds)
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"ranges": args.ranges, "pairs": args.pairs, "points": args.points, "radius_ms": args.radius_ms, "candidates_a_range": total,
              "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    lines = []
    try:
        be.sync_rs_search(cam.kp, c, ranges, track[0], track[1], 0.0, radius_s)          # warm-up: allocations, code object load
        cands = (np.arange(args.cpu_candidates) - args.cpu_candidates // 2) * c.step_s + 0.006
        with tempfile.TemporaryDirectory() as tmp:
            cpu_s, cpu_costs = cpu_loop(tmp, cam, cfg, track, ranges, cands)
        dev_costs = np.array(be.sync_rs_costs(cam.kp, c, ranges, track[0], track[1], [cands] * args.ranges))
        same = bool((dev_costs.view(np.uint64) == cpu_costs.view(np.uint64)).all())
        result.update(cpu_candidates=args.cpu_candidates, cpu_loop_s=cpu_s, cpu_loop_equals_device=same, cpu_loop_scaled_s=cpu_s / args.cpu_candidates * total)
        outs = (torch.zeros((args.ranges, 5), dtype=torch.float64, device=dev),)
        for rep in range(args.reps):
            t0 = time.perf_counter()
            res = be.sync_rs_search(cam.kp, c, ranges, track[0], track[1], 0.0, radius_s)
            wall = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            be.sync_rs_search(cam.kp, c, ranges, track[0], track[1], 0.0, radius_s, out_ptrs=(outs[0].data_ptr(), None, None))
            e1.record(stream)
            e1.synchronize()
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            stream_ms = e0.elapsed_time(e1)
            delays = [r.value * 1000.0 for r in res]
            dev_rows = outs[0].cpu().numpy()
            dev_same = bool(all(dev_rows[i, 3] == res[i].value and dev_rows[i, 4] == res[i].cost for i in range(args.ranges)))
            run = {"wall_s": wall, "stream_ms": stream_ms, "delays_ms": delays, "worst_error_ms": float(max(abs(d - DELAY_S * 1000.0) for d in delays)),
                   "device_output_equals_host_output": dev_same}
            result["runs"].append(run)
            lines.append("run %d: gfw_sync_rs_search of %d ranges x %d pairs x %d points, %d candidates a range: %.3f ms wall with host outputs, %.3f ms on the stream | "
                         "worst |delay - planted| %.4f ms" % (rep, args.ranges, args.pairs, args.points, total, wall * 1e3, stream_ms, run["worst_error_ms"]))
            print(lines[-1], flush=True)
        lines.append("single-threaded C++ loop of the same arithmetic over %d candidates of every range: %.3f s (scaled to %d candidates: %.1f s) | its range costs = "
                     "gfw_sync_rs_costs' to the bit: %s" % (args.cpu_candidates, cpu_s, total, result["cpu_loop_scaled_s"], same))
        print(lines[-1], flush=True)
    finally:
        be.close()
    ok = same and all(r["device_output_equals_host_output"] for r in result["runs"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + json.dumps(result, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
