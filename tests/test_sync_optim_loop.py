"""tools/sync_optim_loop.cpp — the f32 form of the sync-point choice as a single-threaded C++ loop over the library's host-only helpers (gfw_sync_optim_host.h) —
against the f32 statement to the bit, as a shared library; and as a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once on the
200 Hz planted clip from raw samples (resampling included).  No GPU, nothing loaded into python with a sanitizer."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _syncoptimstmt as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "sync_optim_loop.cpp")
OUT = os.path.join(ROOT, "build", "tools")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"


def built(name, extra):
    out = os.path.join(OUT, name)
    deps = [SRC, os.path.join(ROOT, "gyroflow_amd", "csrc", "gfw_sync_optim_host.h"), os.path.join(ROOT, "gyroflow_amd", "csrc", "gfw_layout.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(OUT, exist_ok=True)
        r = subprocess.run([CXX, "-std=c++17", "-ffp-contract=off"] + extra + [SRC, "-o", out + ".%d.tmp" % os.getpid(), "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".%d.tmp" % os.getpid(), out)
    return out


def loop(gyro, rate, target, trims):
    lib = C.CDLL(built("sync_optim_loop.so", ["-O2", "-fPIC", "-shared"]))
    lib.sync_optim_loop.argtypes = [C.c_void_p, C.c_longlong, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 6
    g = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1))
    tr = np.ascontiguousarray(np.asarray(trims, dtype=np.float64).reshape(-1, 2))
    w = S.n_windows(g.shape[1], S.fft_size(rate))
    arr = [np.zeros(w + 1, dtype=np.float32) for _ in range(5)]
    pts = np.zeros(target + 1)
    n = lib.sync_optim_loop(g.ctypes.data, g.shape[1], float(rate), target, tr.ctypes.data if len(tr) else None, len(tr), -1, *[a.ctypes.data for a in arr], pts.ctypes.data)
    return dict(zip(("lf", "mf", "hf", "rank", "rank_nms"), [a[:w] for a in arr]), points=pts[:n])


@pytest.mark.parametrize("i", [0, 1])
def test_the_loop_equals_the_f32_statement_to_the_bit(i):
    rate, dur = S.PLANTED[i]
    g, _ = S.planted_clip(rate, dur)
    got, want = loop(g, rate, 4, [(0.0, dur)]), S.run_f32(g, rate, 4, [(0.0, dur)])
    for k in ("lf", "mf", "hf", "rank", "rank_nms", "points"):
        assert S.same_bits(got[k], want[k]), k
    assert len(got["points"]) >= 3


def test_the_stand_alone_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = built("sync_optim_loop_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSYNC_OPTIM_LOOP_MAIN"])
    g, _ = S.planted_clip(200.0, 60.0)
    n = g.shape[1]
    ts = np.arange(n) * 5.0
    dump = tmp_path / "clip.bin"
    dump.write_bytes(struct.pack("<3q", n, 4, 1) + ts.tobytes() + np.ascontiguousarray(g.T).tobytes() + np.array([0.0, 60.0]).tobytes())
    r = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    gyro, rate = S.resample(ts, g.T)
    want = S.run_f32(gyro, rate, 4, [(0.0, 60.0)])
    assert float.fromhex(words[1]) == rate and int(words[3]) == gyro.shape[1] and int(words[5]) == len(want["rank"])
    pts = np.array([float.fromhex(v) for v in words[10:]])
    assert int(words[9]) == len(pts) and S.same_bits(pts, want["points"])
    fnv = 1469598103934665603
    for b in want["rank"].tobytes():
        fnv = ((fnv ^ b) * 1099511628211) & (2 ** 64 - 1)
    assert words[7] == "%016x" % fnv
