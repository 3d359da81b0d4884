#!/usr/bin/env python3
"""DIS dense optical flow (optical_flow/opencv_dis.rs, the reference's default method 2, without its variational refinement) at the size of a sync: 5 sync points x 46
analysed frames = 225 frame pairs at 1280 x 720, the frames resident in device memory — gfw_flow_dis in one call: wall time with host outputs, and time on the
stream (events around an asynchronous call with device outputs).  Beside it, as the yardstick, gfw_flow_pyrlk in point mode 1 on the same clip: the same grid nodes
tracked by pyramidal Lucas-Kanade.
The frames are tools/flow_bench.py's: crops of one analytic texture shifted by whole pixels from frame to frame, 2 .. 7 px a pair, so the true flow is known.
The first `--check` pairs are compared with the numpy statement of the tests (tests/_disstmt.py) to the bit.  Nothing is timed against the reference, which runs
OpenCV per frame on a thread pool and cannot be built here.
--variational N (N > 0): in the same run, after each unrefined measurement, gfw_flow_dis_refined with N fixed-point iterations a level (the preset: 5; the other
parameters at their defaults) on the same clip — wall, time on the stream, the ratio to the unrefined call of that run, the launches — its first `--check` pairs
compared with tests/_varrefstmt.py to the bit.
usage: dis_bench.py [--groups N] [--frames N] [--width W] [--height H] [--finest 1|2] [--reps R] [--check N] [--variational N] [--out FILE]   (GFW_LIBRARY selects an A/B build.)"""
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
import _disstmt as DS  # noqa: E402
import _varrefstmt as VS  # noqa: E402
import flow_bench as FB  # noqa: E402

DIS_ORDER = ("grid_points", "grid_counts", "flow", "pair_first", "points_a", "points_b")


def streamed(be, dev, call):
    """-> ms on the stream of one asynchronous call with device outputs"""
    import torch
    stream = torch.cuda.current_stream(dev)
    be.set_stream(stream.cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    be.set_option(abi.OPT_SYNCHRONOUS, 1)
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--frames", type=int, default=46)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--finest", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--variational", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    frames, pairs, shifts = FB.clip(args.groups, args.frames, args.width, args.height)
    nodes = warp.flow_grid_nodes(args.width, args.height)
    room = len(pairs) * nodes
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"pairs": len(pairs), "nodes": nodes, "size": [args.width, args.height], "finest_scale": args.finest, "frames": len(frames),
              "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        d_frames = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize(dev)
        be.flow_dis(d_frames.data_ptr(), args.width, pairs, args.finest, shape=frames.shape)           # warm-up: allocations, code object load
        be.flow_pyrlk(d_frames.data_ptr(), args.width, pairs, None, shape=frames.shape)
        t0 = time.perf_counter()
        want = DS.flow_dis(frames, pairs[:args.check], args.finest)
        stmt_s = (time.perf_counter() - t0) / max(args.check, 1)
        if args.variational:
            be.flow_dis(d_frames.data_ptr(), args.width, pairs, args.finest, shape=frames.shape, variational_iters=args.variational)      # warm-up: the larger work space
            ref = VS.DEFAULT._replace(fixed_point_iters=args.variational)
            want_ref = VS.flow_dis_refined(frames, pairs[:args.check], args.finest, ref)
            levels = DS.coarsest_scale(args.width, args.height) - args.finest + 1
            result["variational_iters"] = args.variational
            result["launches"] = {"unrefined": 3 + DS.coarsest_scale(args.width, args.height) + 4 * levels,
                                  "refined": 3 + DS.coarsest_scale(args.width, args.height) + (4 + 2 + ref.fixed_point_iters * (1 + 2 * ref.sor_iters)) * levels}
        z = lambda shape, t: torch.zeros(shape, dtype=t, device=dev)
        dis_outs = {"grid_points": None, "grid_counts": None, "flow": None, "pair_first": z(len(pairs) + 1, torch.int32), "points_a": z((room, 2), torch.float32),
                    "points_b": z((room, 2), torch.float32)}
        lk_outs = {"next": z((room, 2), torch.float32), "status": z(room, torch.uint8), "iters": None, "grid_points": None, "grid_counts": None,
                   "pair_first": z(len(pairs) + 1, torch.int32), "points_a": z((room, 2), torch.float32), "points_b": z((room, 2), torch.float32)}
        true = np.array(shifts, dtype=np.float32)
        for rep in range(args.reps):
            t0 = time.perf_counter()
            got = be.flow_dis(d_frames.data_ptr(), args.width, pairs, args.finest, flow=rep == 0, shape=frames.shape)
            wall = time.perf_counter() - t0
            dis_ms = streamed(be, dev, lambda: be.flow_dis(d_frames.data_ptr(), args.width, pairs, args.finest,
                                                           out_ptrs=tuple(None if dis_outs[n] is None else dis_outs[n].data_ptr() for n in DIS_ORDER), shape=frames.shape))
            t0 = time.perf_counter()
            lk = be.flow_pyrlk(d_frames.data_ptr(), args.width, pairs, None, shape=frames.shape)
            lk_wall = time.perf_counter() - t0
            lk_ms = streamed(be, dev, lambda: be.flow_pyrlk(d_frames.data_ptr(), args.width, pairs, None,
                                                            out_ptrs=tuple(None if lk_outs[n] is None else lk_outs[n].data_ptr() for n in FB.ORDER), shape=frames.shape))
            first = got["pair_first"]
            err = np.concatenate([np.linalg.norm((got["points_b"][first[p]:first[p + 1]] - got["points_a"][first[p]:first[p + 1]]) - true[p], axis=1) for p in range(len(pairs))])
            lf = lk["pair_first"]
            lk_err = np.concatenate([np.linalg.norm((lk["points_b"][lf[p]:lf[p + 1]] - lk["points_a"][lf[p]:lf[p + 1]]) - true[p], axis=1) for p in range(len(pairs))])
            k = int(want["pair_first"][-1])
            same = got["points_a"][:k].tobytes() == want["points_a"].tobytes() and got["points_b"][:k].tobytes() == want["points_b"].tobytes() and \
                first[:args.check + 1].tobytes() == want["pair_first"].tobytes() and (rep != 0 or got["flow"][:args.check].tobytes() == want["flow"].tobytes())
            run = {"wall_s": wall, "stream_ms": dis_ms, "pyrlk_grid_wall_s": lk_wall, "pyrlk_grid_stream_ms": lk_ms, "statement_s_per_pair": stmt_s, "device_equals_statement": bool(same),
                   "device_output_equals_host_output": dis_outs["points_b"].cpu().numpy()[:int(first[-1])].tobytes() == got["points_b"].tobytes(),
                   "points": int(first[-1]), "median_error_px": float(np.median(err)), "p99_error_px": float(np.percentile(err, 99)),
                   "pyrlk_kept": int(lf[-1]), "pyrlk_median_error_px": float(np.median(lk_err))}
            if args.variational:
                t0 = time.perf_counter()
                rgot = be.flow_dis(d_frames.data_ptr(), args.width, pairs, args.finest, flow=rep == 0, shape=frames.shape, variational_iters=args.variational)
                rwall = time.perf_counter() - t0
                ref_ms = streamed(be, dev, lambda: be.flow_dis(d_frames.data_ptr(), args.width, pairs, args.finest, variational_iters=args.variational,
                                                               out_ptrs=tuple(None if dis_outs[n] is None else dis_outs[n].data_ptr() for n in DIS_ORDER), shape=frames.shape))
                rfirst = rgot["pair_first"]
                rerr = np.concatenate([np.linalg.norm((rgot["points_b"][rfirst[p]:rfirst[p + 1]] - rgot["points_a"][rfirst[p]:rfirst[p + 1]]) - true[p], axis=1) for p in range(len(pairs))])
                rsame = rgot["points_a"][:k].tobytes() == want_ref["points_a"].tobytes() and rgot["points_b"][:k].tobytes() == want_ref["points_b"].tobytes() and \
                    rfirst[:args.check + 1].tobytes() == want_ref["pair_first"].tobytes() and (rep != 0 or rgot["flow"][:args.check].tobytes() == want_ref["flow"].tobytes())
                run.update(refined_wall_s=rwall, refined_stream_ms=ref_ms, refined_over_unrefined=ref_ms / dis_ms, refined_equals_statement=bool(rsame),
                           refined_device_output_equals_host_output=dis_outs["points_b"].cpu().numpy()[:int(rfirst[-1])].tobytes() == rgot["points_b"].tobytes(),
                           refined_median_error_px=float(np.median(rerr)), refined_p99_error_px=float(np.percentile(rerr, 99)))
                print("run %d: gfw_flow_dis_refined, %d fixed-point iterations a level: %.3f ms wall with host outputs, %.3f ms on the stream = %.3f x the unrefined call "
                      "(+ %.3f ms), %d launches instead of %d | device = statement on %d pairs: %s | error against the true shift: median %.4f px, 99 %% %.4f px" %
                      (rep, args.variational, rwall * 1e3, ref_ms, ref_ms / dis_ms, ref_ms - dis_ms, result["launches"]["refined"], result["launches"]["unrefined"], args.check,
                       rsame, run["refined_median_error_px"], run["refined_p99_error_px"]), flush=True)
            result["runs"].append(run)
            print("run %d: gfw_flow_dis of %d pairs at %d x %d, finest scale %d: %.3f ms wall with host outputs, %.3f ms on the stream | gfw_flow_pyrlk on the same grid "
                  "(%d nodes a frame): %.3f ms wall, %.3f ms on the stream | the numpy statement %.2f s a pair | device = statement on %d pairs: %s | %d points, error "
                  "against the true shift: median %.4f px, 99 %% %.4f px (PyrLK: %d kept, median %.4f px)" %
                  (rep, len(pairs), args.width, args.height, args.finest, wall * 1e3, dis_ms, nodes, lk_wall * 1e3, lk_ms, stmt_s, args.check, same, run["points"],
                   run["median_error_px"], run["p99_error_px"], run["pyrlk_kept"], run["pyrlk_median_error_px"]), flush=True)
    finally:
        be.close()
    ok = all(r["device_equals_statement"] and r["device_output_equals_host_output"] and r.get("refined_equals_statement", True) and
             r.get("refined_device_output_equals_host_output", True) for r in result["runs"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
