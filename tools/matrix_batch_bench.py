#!/usr/bin/env python3
"""The per-row matrix builder for a clip with IBIS/OIS splines: 64 frames of a 4K clip (2160 rows each, 19 control points per spline), three ways, timed with
hipEvents on the context's stream (asynchronous context, caller-owned tables for the per-frame entry so that its builds are in order on that stream):
  (a) 64 gfw_build_matrices_stab calls, one per frame;
  (b) one gfw_build_matrices_batch_stab call of 64;
  (c) one gfw_build_matrices_batch call of the same frames without stabiliser data.
Prints the stream time and the host wall time of each, per frame, and checks that (a) and (b) wrote the same bits.
usage: matrix_batch_bench.py [--reps R] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gyroflow_amd import abi, synthetic as S, warp  # noqa: E402

W, H, READOUT, N = 3840, 2160, 16.0, 64


def stab_for(k):
    pos = np.linspace(-200.0, 3900.0, 19)
    ph = 0.37 * k
    ibis = np.stack([pos, 40.0 * np.sin(pos * 0.004 + ph), -40.0 * np.cos(pos * 0.003 - ph), 100.0 * np.sin(pos * 0.002 + 0.4 + ph)], axis=1)
    ois = np.stack([pos, 15.0 * np.cos(pos * 0.005 - ph), 15.0 * np.sin(pos * 0.006 + ph), np.zeros_like(pos)], axis=1)
    return {"offset": 12.5, "sensor_size": (6000.0, 3376.0), "crop_area": (120.0, 68.0, 5760.0, 3240.0), "pixel_pitch": (3.0, 3.0),
            "width": float(W), "height": float(H), "ibis": ibis, "ois": ois}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    org = S.sampled_track_fast(11, 0.0, 4000.0, 500.0)
    smo = S.sampled_track_fast(12, 0.0, 4000.0, 100.0, scale=0.25)
    lens = S.gopro_style_lens(W, H)
    nk = np.asarray(S.new_k(lens, 1.0, W, H), dtype=np.float64).reshape(9)
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1, lens=lens)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    timings = (abi.FrameTiming * N)()
    for k in range(N):
        t = timings[k]
        t.timestamp_ms, t.frame_readout_time_ms, t.rows, t.readout_dim = 1000.0 + 33.3 * k, READOUT, H, H
        for i in range(9):
            t.new_k[i] = nk[i]
    stabs = [stab_for(k) for k in range(N)]
    table, keep = warp.frame_stab_table(stabs)
    structs = [kp[0] for kp in keep]
    own = torch.zeros((N, H, 16), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * N)()
    lib, ctx = be.lib, be.ctx
    result = {"frames": N, "rows": H, "runs": []}

    def timed(fn):
        stream = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        host = time.perf_counter() - t0
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0, host * 1e6                      # us on the stream, us of host time until the last call returned

    def per_frame():
        for k in range(N):
            be._check(lib.gfw_build_matrices_stab(ctx, C.byref(timings[k]), C.byref(structs[k]), own[k].data_ptr(), None))

    def batch_stab():
        be._check(lib.gfw_build_matrices_batch_stab(ctx, timings, table, N, ptrs))

    def batch_plain():
        be._check(lib.gfw_build_matrices_batch(ctx, timings, N, ptrs))
    try:
        be.set_quaternion_tracks(org, smo)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        for fn in (per_frame, batch_stab, batch_stab, batch_plain, batch_plain):       # warm-up: allocations of both alternating batches, code object load
            fn()
        be.synchronize()
        batch_stab()
        be.synchronize()
        hip = C.CDLL("libamdhip64.so")
        got = np.empty((N, H, 16), dtype=np.float32)
        for k in range(N):
            assert hip.hipMemcpy(C.c_void_p(got[k].ctypes.data), C.c_void_p(ptrs[k]), C.c_size_t(got[k].nbytes), 2) == 0
        same = bool(np.array_equal(got.view(np.uint32), own.cpu().numpy().view(np.uint32)))
        result["batch_equals_per_frame_bits"] = same
        for rep in range(args.reps):
            a, b, c = timed(per_frame), timed(batch_stab), timed(batch_plain)
            result["runs"].append({"per_frame_stream_us": a[0], "per_frame_host_us": a[1], "batch_stab_stream_us": b[0], "batch_stab_host_us": b[1],
                                   "batch_plain_stream_us": c[0], "batch_plain_host_us": c[1]})
            print("run %d, 64 frames: gfw_build_matrices_stab x 64: %.1f us on the stream (%.2f us per frame), host %.1f us | gfw_build_matrices_batch_stab: %.1f us "
                  "(%.2f per frame), host %.1f us | gfw_build_matrices_batch (no stabiliser data): %.1f us (%.2f per frame), host %.1f us"
                  % (rep, a[0], a[0] / N, a[1], b[0], b[0] / N, b[1], c[0], c[0] / N, c[1]), flush=True)
    finally:
        be.close()
    print("batch tables equal the per-frame entry's bit for bit: %s" % same)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
