#!/usr/bin/env python3
"""The gyro-match offset search (find_offset/essential_matrix.rs:13-131) at its default size — 5 ranges of 90 estimated samples (1.5 s at 60 fps), a 1 kHz gyro cut
to each range's window, search_size 5000 ms (cli.rs: 5 s): 10 000 coarse + 200 fine candidates a range — three ways:
  (a) gfw_sync_gyro_search in one call with host outputs (wall time: staging, upload, four launches, download), and the time on the stream alone from hipEvents
      around an asynchronous call with device outputs;
  (b) the same search as a plain single-threaded C++ loop on the host (tools/sync_gyro_loop.cpp, built here with g++ -O2);
  (c) the numpy statement of the tests (tests/_syncgyrostmt.py).
The three results are compared to the bit.  (b) and (c) are context, not a pass mark: the reference runs this search under rayon on all host cores and cannot be
built here.  usage: sync_gyro_bench.py [--ranges N] [--search-size MS] [--reps R] [--out FILE]   (GFW_LIBRARY selects an A/B build of the library.)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402
import _syncgyrostmt as G  # noqa: E402


def loop_library():
    src, out = os.path.join(ROOT, "tools", "sync_gyro_loop.cpp"), os.path.join(ROOT, "build", "tools", "sync_gyro_loop.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", out])
    lib = C.CDLL(out)
    lib.sync_gyro_loop.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_double, C.c_double, C.c_void_p]
    lib.sync_gyro_loop.restype = None
    return lib


def workload(n_ranges, search_size):
    c = G.Clip(60.0, 1000.0, -271.83, seed=77, duration_s=10.0 + 4.0 * n_ranges, span=[(6.0 + 4.0 * k, 7.5 + 4.0 * k) for k in range(n_ranges)])
    ins = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, search_size)
    return c, [(r["est"], r["est_has"], r["gyro"], r["gyro_has"]) for r in ins]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranges", type=int, default=5)
    ap.add_argument("--search-size", type=float, default=5000.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    clip, ranges = workload(args.ranges, args.search_size)
    n = len(ranges)
    n_coarse = warp.sync_gyro_coarse_count(args.search_size)
    ef, e, eh, gf, g, gh = warp.Backend._sync_gyro_ranges(ranges)
    loop = loop_library()
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"ranges": n, "estimated_samples": [len(r[0]) for r in ranges], "gyro_samples": [len(r[2]) for r in ranges], "search_size_ms": args.search_size,
              "candidates_per_range": n_coarse + abi.SYNC_FINE_CANDIDATES, "library": os.environ.get("GFW_LIBRARY", ""), "runs": []}
    try:
        be.sync_gyro_search(ranges, 0.0, args.search_size)                    # warm-up: allocations, code object load
        d_res = torch.zeros(n * 5, dtype=torch.float64, device=dev)
        for rep in range(args.reps):
            t0 = time.perf_counter()
            res = be.sync_gyro_search(ranges, 0.0, args.search_size)
            wall = time.perf_counter() - t0
            stream = torch.cuda.current_stream(dev)
            be.set_stream(stream.cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            be.sync_gyro_search(ranges, 0.0, args.search_size, result_ptr=d_res.data_ptr())
            e1.record(stream)
            e1.synchronize()
            be.set_option(abi.OPT_SYNCHRONOUS, 1)
            out = np.zeros((n, 4))
            t0 = time.perf_counter()
            loop.sync_gyro_loop(ef.ctypes.data, e.ctypes.data, eh.ctypes.data, gf.ctypes.data, g.ctypes.data, gh.ctypes.data, n, 0.0, args.search_size, out.ctypes.data)
            wall_loop = time.perf_counter() - t0
            t0 = time.perf_counter()
            stated = [G.search(a, b, c_, d, 0.0, args.search_size) for a, b, c_, d in ranges]
            wall_numpy = time.perf_counter() - t0
            dev_rows = np.array([[r.coarse_value, r.coarse_cost, r.value, r.cost] for r in res])
            run = {"search_wall_s": wall, "search_stream_ms": e0.elapsed_time(e1), "cpp_loop_s": wall_loop, "numpy_statement_s": wall_numpy,
                   "device_equals_cpp_loop": dev_rows.tobytes() == out.tobytes(),
                   "device_equals_statement": dev_rows.tobytes() == np.array([[s["coarse_value"], s["coarse_cost"], s["value"], s["cost"]] for s in stated]).tobytes(),
                   "device_output_equals_host_output": d_res.cpu().numpy().tobytes() == b"".join(bytes(r) for r in res),
                   "offsets_ms": [r.value for r in res], "planted_ms": clip.offset_ms}
            result["runs"].append(run)
            print("run %d: gfw_sync_gyro_search of %d ranges x %d candidates: %.3f ms wall with host outputs, %.3f ms on the stream | the C++ loop %.1f ms | the numpy statement "
                  "%.0f ms | device = C++ loop: %s, = statement: %s" % (rep, n, n_coarse + abi.SYNC_FINE_CANDIDATES, wall * 1e3, run["search_stream_ms"], wall_loop * 1e3,
                                                                         wall_numpy * 1e3, run["device_equals_cpp_loop"], run["device_equals_statement"]), flush=True)
    finally:
        be.close()
    ok = all(r["device_equals_cpp_loop"] and r["device_equals_statement"] and r["device_output_equals_host_output"] for r in result["runs"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
