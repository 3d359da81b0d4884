"""gyroflow::OptimSync (include/gfwarp.hpp: where in a clip to sync, over gfw_optim_resample + gfw_sync_optim_points) driven by a C++ program
(tests/cpp/test_sync_optim.cpp) against a dump of the numpy statements' results (tests/_syncoptimstmt.py) for the 200 Hz planted clip with jittered timestamps and
a few missing gyro values.  CPU: make() equals the statement's resampling to the bit, nullopt without samples, the loud failure without a context.  GPU: run()'s
points, rank and ratio equal the f32 statement's to the bit."""
import os
import subprocess

import numpy as np
import pytest

import _syncoptimstmt as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_sync_optim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sync_optim.cpp"), "-o", out,
                           "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """raw samples, the statement's resampled series, its points, rank and ratio, as text"""
    g, centres = S.planted_clip(200.0, 60.0)
    n = g.shape[1]
    rs = np.random.RandomState(5)
    ts = np.sort(5.0 * (np.arange(n) + rs.uniform(-0.2, 0.2, n)))
    has = np.ones(n, dtype=np.uint8)
    has[[3, 4, 50, 51]] = 0                                                             # in the quiet lead-in
    gyro, rate = S.resample(ts, g.T, has)
    want = S.run_f32(gyro, rate, 4, [(0.0, 60.0)])
    assert len(want["points"]) == 4 and S.fft_size(rate) == 200
    lines = [str(n)] + ["%s %d %s %s %s" % (h(ts[i]), has[i], h(g[0, i]), h(g[1, i]), h(g[2, i])) for i in range(n)]
    lines += [h(rate), str(gyro.shape[1])] + [h(v) for v in gyro.reshape(-1)]
    lines += ["4", "1", "%s %s" % (h(0.0), h(60.0))]
    lines += [str(len(want["points"]))] + [h(v) for v in want["points"]]
    lines += [str(len(want["rank"]))] + [h(v) for v in want["rank"]] + [h(want["ratio"])]
    path = str(tmp_path_factory.mktemp("sync_optim") / "clip.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_cpp_optim_sync_host_half(exe, dump):
    out = subprocess.run([exe, "validate", dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok:" in out.stdout


@pytest.mark.gpu
def test_cpp_optim_sync_on_the_device(exe, dump):
    out = subprocess.run([exe, "run", dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "run ok: 4 points" in out.stdout
