#!/usr/bin/env python3
"""The visual-features offset search (find_offset/visual_features.rs:10-147) of one range — a 4K clip with a 16 ms readout, 60 matched frame pairs of 400 points,
search_size 5000 ms (the reference's default: cli.rs:623, 5 s), so 5000 coarse + 200 fine candidates — two ways:
  (a) through the ABI without gfw_sync_visual_search: per candidate, pair and side the rotations of the points on the host (f64 slerp over the tracks,
      numpy-vectorised over the points), one synchronous gfw_undistort_points call, the fold on the host.  Run for --candidates-a candidates and extrapolated to the
      search; the time spent INSIDE the gfw_undistort_points calls is reported on its own, so that the host-side Python of this tool can be told from what any
      caller of that ABI pays;
  (b) gfw_sync_visual_search in one call (host outputs: wall time includes the upload and the download), and the time on the stream alone from hipEvents around an
      asynchronous call with device outputs.
For the subset of route (a) the two routes' costs are compared (gfw_sync_visual_costs on the same candidates).
usage: sync_bench.py [--pairs N] [--points N] [--search-size MS] [--candidates-a M] [--reps R] [--out FILE]   (GFW_LIBRARY selects an A/B build of the library.)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402
import zoom_bench as ZB  # noqa: E402

W, H, READOUT = ZB.W, ZB.H, ZB.READOUT


def fold(p1, p2):
    """visual_features.rs:66-81 for one pair"""
    ok = (p1[:, 0] > 0) & (p1[:, 0] < np.float32(W)) & (p1[:, 1] > 0) & (p1[:, 1] < np.float32(H)) & (p2[:, 0] > 0) & (p2[:, 0] < np.float32(W)) & (p2[:, 1] > 0) & (p2[:, 1] < np.float32(H))
    dx, dy = p2[ok, 0] - p1[ok, 0], p2[ok, 1] - p1[ok, 1]
    d = np.sort(((dx * dx) + (dy * dy)).astype(np.uint64))
    return int(d[:int(float(len(d)) * 0.9)].sum(dtype=np.uint64))


def route_a(be, kp, org, smo, nk, pairs, candidates):
    """-> (costs, seconds inside gfw_undistort_points, calls)"""
    costs, t_calls, calls = [], 0.0, 0
    for offs, _ in candidates:
        total = 0
        for ts, next_ts, p, q in pairs:
            mapped = []
            for t_us, pts in ((ts, p), (next_ts, q)):
                rot = ZB.rotations_for(org, smo, nk, float(t_us) / 1000.0 - offs, pts)
                t0 = time.perf_counter()
                mapped.append(be.undistort_points(kp, rot, points=pts, index_mode=abi.POINT_INDEX_PER_POINT))
                t_calls += time.perf_counter() - t0
                calls += 1
            total += fold(mapped[0], mapped[1])
        costs.append(float(total))
    return np.array(costs), t_calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=60)
    ap.add_argument("--points", type=int, default=400)
    ap.add_argument("--search-size", type=float, default=5000.0)
    ap.add_argument("--candidates-a", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = np.random.default_rng(17)
    t_end = 1000.0 + 66.7 * args.pairs + 400.0
    half = args.search_size / 2.0 + 50.0
    org = S.sampled_track_fast(11, 1000.0 - half, t_end + half, 500.0)
    smo = S.sampled_track_fast(12, 1000.0 - half, t_end + half, 100.0, scale=0.25)
    lens = S.gopro_style_lens(W, H)
    nk = S.new_k(lens, 1.0, W, H)
    kp = S.base_kernel_params(lens, 1.0, 1)
    kp.width, kp.height, kp.output_width, kp.output_height = W, H, W, H
    pairs = []
    for k in range(args.pairs):
        p = np.stack([g.uniform(0.1 * W, 0.9 * W, args.points), g.uniform(0.1 * H, 0.9 * H, args.points)], 1).astype(np.float32)
        q = (p + g.normal(0.0, 6.0, p.shape)).astype(np.float32)
        t = int(round((1200.0 + 66.7 * k) * 1000.0))
        pairs.append((t, t + 66667, p, q))
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1, lens=lens)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    search = abi.SyncSearch(width=W, height=H)
    for i, v in enumerate(nk.reshape(9)):
        search.new_k[i] = v
    n_coarse = warp.sync_coarse_count(0, args.search_size, 30.0)
    coarse = np.array([(0.0 + (-(args.search_size / 2.0) + float(i)), READOUT) for i in range(n_coarse)], dtype=np.float64).reshape(-1, 2)
    subset = coarse[np.linspace(0, n_coarse - 1, min(args.candidates_a, n_coarse)).astype(int)] if n_coarse else coarse
    n_all = n_coarse + abi.SYNC_FINE_CANDIDATES
    result = {"pairs": args.pairs, "points": args.points, "search_size_ms": args.search_size, "candidates": n_all, "candidates_a": len(subset),
              "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}

    def search_all(**kw):
        return be.sync_visual_search(kp, search, pairs, 0, 0.0, args.search_size, READOUT, **kw)
    try:
        be.set_quaternion_tracks(org, smo)
        search_all()                                                          # warm-up: allocations, code object load
        route_a(be, kp, org, smo, nk, pairs[:2], subset[:1])
        d_res = torch.zeros(5, dtype=torch.float64, device=dev)
        d_costs = torch.zeros(max(n_coarse, 1), dtype=torch.float64, device=dev)
        for rep in range(args.reps):
            t0 = time.perf_counter()
            ca, t_calls, calls = route_a(be, kp, org, smo, nk, pairs, subset)
            wall_a = time.perf_counter() - t0
            cb = be.sync_visual_costs(kp, search, pairs, subset)
            t0 = time.perf_counter()
            res = search_all()
            wall_b = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(stream)
            search_all(result_ptr=d_res.data_ptr())
            e1.record(stream)
            be.sync_visual_costs(kp, search, pairs, coarse, out_ptr=d_costs.data_ptr())
            e2.record(stream)
            e2.synchronize()
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            scale = n_all / max(len(subset), 1)
            run = {"a_wall_s": wall_a, "a_inside_calls_s": t_calls, "a_calls": calls, "a_extrapolated_s": wall_a * scale, "a_calls_extrapolated_s": t_calls * scale,
                   "b_wall_s": wall_b, "b_stream_ms": e0.elapsed_time(e1), "coarse_costs_stream_ms": e1.elapsed_time(e2), "b_candidates_per_s": n_all / wall_b,
                   "max_cost_difference": float(np.max(np.abs(ca - cb))) if len(subset) else 0.0, "max_cost": float(np.max(cb)) if len(subset) else 0.0,
                   "device_matches_host_output": d_res.cpu().numpy().tobytes() == bytes(res), "value_ms": res.value, "cost": res.cost}
            result["runs"].append(run)
            print("run %d: (a) %d candidates %.3f s (%.3f s inside %d gfw_undistort_points calls) -> %.1f s (%.1f s) for %d candidates | "
                  "(b) %d candidates %.4f s wall, %.3f ms on the stream; the coarse costs alone %.3f ms | costs of the subset differ by at most %g (of %g)"
                  % (rep, len(subset), wall_a, t_calls, calls, run["a_extrapolated_s"], run["a_calls_extrapolated_s"], n_all, n_all, wall_b, run["b_stream_ms"],
                     run["coarse_costs_stream_ms"], run["max_cost_difference"], run["max_cost"]), flush=True)
    finally:
        be.close()
    ok = all(r["b_wall_s"] < r["a_calls_extrapolated_s"] for r in result["runs"])
    print("gfw_sync_visual_search of %d candidates takes less wall time than the gfw_undistort_points calls of route (a) alone, extrapolated: %s" % (n_all, ok))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
