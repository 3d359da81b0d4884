#!/usr/bin/env python3
"""The choice of a clip's sync points (optimsync.rs; gfw_sync_optim_points) on 10-minute clips with a 200 Hz, a 1 kHz and a 4 kHz gyro:
  (a) gfw_sync_optim_points with host outputs (wall time: the f32 cast, staging, upload, six launches, download), and the time on the stream alone from hipEvents
      around an asynchronous call with device outputs — three times each;
  (b) the f32 form as a plain single-threaded C++ loop on the host (tools/sync_optim_loop.cpp, built here with g++ -O2 -ffp-contract=off).  The direct form is
      O(fft_size^2) a window, so on the larger clips the loop does the first windows only, as many as --loop-macs allows, and their time is scaled to the clip
      (printed as such); the device's band energies of those windows — or, where the loop ran the whole clip, everything down to the points — are compared to the
      loop's to the bit;
  (c) the literal f64 statement of the tests with numpy.fft (tests/_syncoptimstmt.py: run_literal) on the host, whole clip (not at 4 kHz: it holds every
      window's transform at once).
(b) and (c) are context, not a pass mark: the reference runs rustfft, an O(N log N) transform, and cannot be built here.  Expect the direct form to scale with the
square of the rate: an 8 kHz gyro is 64 x the work of a 1 kHz one per second of clip — seconds, not milliseconds.
usage: sync_optim_bench.py [--rates 200,1000,4000] [--seconds 600] [--reps 3] [--loop-macs 1e10] [--out FILE]   (GFW_LIBRARY selects an A/B build of the library.)"""
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

from gyroflow_amd import abi, synthetic as SF, warp  # noqa: E402
import _syncoptimstmt as S  # noqa: E402


def loop_library():
    src, out = os.path.join(ROOT, "tools", "sync_optim_loop.cpp"), os.path.join(ROOT, "build", "tools", "sync_optim_loop.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", out])
    lib = C.CDLL(out)
    lib.sync_optim_loop.argtypes = [C.c_void_p, C.c_longlong, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 6
    return lib


def clip(rate, seconds):
    """noise and a burst every 40 s"""
    rs = np.random.RandomState(int(rate))
    s = int(rate * seconds)
    t = np.arange(s) / rate
    g = rs.normal(0.0, 0.3, (3, s))
    for c in np.arange(15.0, seconds - 10.0, 40.0):
        env = np.exp(-0.5 * ((t - c) / 0.8) ** 2)
        for a in range(3):
            g[a] += 50.0 * env * np.sin(2.0 * np.pi * 7.0 * t + a * 2.0 * np.pi / 3.0)
    return np.ascontiguousarray(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", default="200,1000,4000")
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--target", type=int, default=10)
    ap.add_argument("--loop-macs", type=float, default=1e10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    loop = loop_library()
    fr = SF.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    result = {"seconds": args.seconds, "target_sync_points": args.target, "library": os.environ.get("GFW_LIBRARY", ""), "clips": []}
    ok = True
    try:
        for rate in [float(r) for r in args.rates.split(",")]:
            g = clip(rate, args.seconds)
            s = g.shape[1]
            n = S.fft_size(rate)
            w = S.n_windows(s, n)
            trims = [(0.0, args.seconds)]
            tr = np.array(trims)
            be.sync_optim_points(g, rate, args.target, trims)                      # warm-up: allocations, code object load
            d_pts = torch.zeros(args.target, dtype=torch.float64, device=dev)
            d_n = torch.zeros(1, dtype=torch.int32, device=dev)
            runs = []
            for rep in range(args.reps):
                t0 = time.perf_counter()
                pts, rank, ratio, nms = be.sync_optim_points(g, rate, args.target, trims, details=True)
                wall = time.perf_counter() - t0
                stream = torch.cuda.current_stream(dev)
                be.set_stream(stream.cuda_stream)
                be.set_option(abi.OPT_SYNCHRONOUS, 0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                be.sync_optim_points(g, rate, args.target, trims, out_ptrs=(d_pts.data_ptr(), d_n.data_ptr(), None, None))
                e1.record(stream)
                e1.synchronize()
                be.set_option(abi.OPT_SYNCHRONOUS, 1)
                runs.append({"points_wall_s": wall, "points_stream_ms": e0.elapsed_time(e1),
                             "device_output_equals_host_output": d_pts.cpu().numpy()[:int(d_n.cpu()[0])].tobytes() == pts.tobytes()})
            lf, mf, hf, rank2 = be.sync_optim_rank(g, rate)
            per_window = 3.0 * n * (n // 2 + 1)
            lw = w if per_window * w <= args.loop_macs else max(int(args.loop_macs / per_window), 1)
            arr = [np.zeros(w + 1, dtype=np.float32) for _ in range(5)]
            lpts = np.zeros(args.target + 1)
            t0 = time.perf_counter()
            ln = loop.sync_optim_loop(g.ctypes.data, s, rate, args.target, tr.ctypes.data, 1, lw if lw < w else -1, *[a.ctypes.data for a in arr], lpts.ctypes.data)
            loop_s = time.perf_counter() - t0
            same = all(a[:lw].tobytes() == b[:lw].tobytes() for a, b in zip(arr[:3], (lf, mf, hf)))
            if lw == w:
                same = same and arr[3][:w].tobytes() == rank.tobytes() and arr[4][:w].tobytes() == nms.tobytes() and lpts[:ln].tobytes() == pts.tobytes()
            numpy_s, lit_same = None, None
            if w * n <= 5e7:                                                        # (the statement holds every window's transform at once: 16 bytes a point)
                t0 = time.perf_counter()
                lit = S.run_literal(g, rate, args.target, trims)
                numpy_s = time.perf_counter() - t0
                lit_same = lit["points"].tobytes() == pts.tobytes()
            c = {"rate_hz": rate, "samples": s, "fft_size": n, "windows": w, "runs": runs, "loop_windows": lw, "loop_s": loop_s, "loop_scaled_to_clip_s": loop_s * w / lw,
                 "device_equals_cpp_loop": bool(same), "numpy_fft_f64_statement_s": numpy_s, "points_ms": pts.tolist(),
                 "points_equal_literal_statement": lit_same, "rank_equals_rank_entry": rank2.tobytes() == rank.tobytes()}
            ok = ok and same and c["rank_equals_rank_entry"] and all(r["device_output_equals_host_output"] for r in runs)
            result["clips"].append(c)
            print("%g Hz, %d samples, fft_size %d, %d windows: gfw_sync_optim_points %s ms wall with host outputs, %s ms on the stream | the C++ loop %.2f s for %d windows "
                  "(%.1f s scaled to the clip) | numpy.fft f64 statement %s | device = C++ loop: %s | points = literal statement's: %s"
                  % (rate, s, n, w, "/".join("%.2f" % (r["points_wall_s"] * 1e3) for r in runs), "/".join("%.2f" % r["points_stream_ms"] for r in runs), loop_s, lw,
                     c["loop_scaled_to_clip_s"], "not run (memory)" if numpy_s is None else "%.2f s" % numpy_s, same, c["points_equal_literal_statement"]), flush=True)
    finally:
        be.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
