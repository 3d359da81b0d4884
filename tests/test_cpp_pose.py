"""gyroflow::estimate_poses_almeida / estimated_gyro (include/gfwarp.hpp: Almeida pose estimation over gfw_pose_almeida and the series made of its rotations) driven by
a C++ program (tests/cpp/test_pose.cpp) against a dump of the numpy statement's results (tests/_posestmt.py) under the library's own draws (gfw_pose_draws: host
code).  CPU: pairs without points, the loud failure without a context, scaled_axis, and estimated_gyro equal to the Python mirror's to the bit.  GPU: quaternions,
rotations and best rounds equal to the statement's to the bit; euler within 1e-12 (the same f64 formula through two math libraries' acos)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gyroflow_amd import synchronization as SY, warp
import _posecase as PC
import _posestmt as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")
SEED, FPS, NTH = 20241, 59.94, 2.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_pose")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pose.cpp"), "-o", out, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


def frames():
    """{timestamp_us: euler or None}: 12 analysed frames, two without a rotation (one inside, one at the end)"""
    g = np.random.default_rng(5)
    out = {}
    for k in range(12):
        out[1000000 + 33367 * k] = None if k in (4, 11) else tuple(float(v) for v in g.uniform(-0.4, 0.4, 3))
    return out


def stated_pairs():
    """the pairs of the fisheye case (None in front and inside), and what the statement makes of them under the library's draws for SEED"""
    c = PC.case("fisheye-r7")
    pairs = [None] + list(c.pairs[3:6]) + [None] + list(c.pairs[6:8])
    live = [p for p in pairs if p is not None]
    triples, samples = warp.pose_draws(SEED, [len(a) for a, _ in live], c.cam.num_iters, c.cam.num_samples)
    quats, rot, best, _, _ = PS.estimate(c.cam, live, triples, samples)
    want, k = [], 0
    for p in pairs:
        if p is None:
            want.append(None)
        else:
            want.append(dict(quat=quats[k], rotation=rot[k], best=best[k], euler=SY.scaled_axis(rot[k]) * (FPS / NTH)))
            k += 1
    return c, pairs, want


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    c, pairs, want = stated_pairs()
    cam = c.cam
    cfg = PC.cfg_of(cam)
    lines = [bytes(cam.kp).hex(), "%d %d" % (cam.clip.model, cam.clip.digital),
             "%d %d %d %d %d %d %s %s" % (cfg.video_width, cfg.video_height, cfg.flow_width, cfg.flow_height, cfg.num_iters, cfg.num_samples, h(cfg.inlier_angle_deg),
                                          " ".join(h(cfg.camera_matrix[i]) for i in range(9))),
             "%s %s %d" % (h(FPS), h(NTH), SEED), str(len(pairs))]
    for p, w in zip(pairs, want):
        if p is None:
            lines += ["0 0", "0 " + " ".join([h(0.0)] * 16) + " 0 -1"]
            continue
        a, b = p
        lines.append("1 %d" % len(a))
        lines += ["%s %s %s %s" % (h(x[0]), h(x[1]), h(y[0]), h(y[1])) for x, y in zip(a, b)]
        lines.append("1 " + " ".join(h(v) for v in list(w["quat"]) + list(w["rotation"].reshape(9)) + list(w["euler"])) + " %d %d" % tuple(w["best"]))
    res = frames()
    lines.append(str(len(res)))
    lines += ["%d %d %s %s %s" % ((k, 0, h(0.0), h(0.0), h(0.0)) if e is None else (k, 1, h(e[0]), h(e[1]), h(e[2]))) for k, e in sorted(res.items())]
    gyro = SY.estimated_gyro(res, FPS, 10.0, True)
    lines.append("%s %s 1" % (h(FPS), h(10.0)))
    lines.append(str(len(gyro)))
    lines += ["%d %s %s %s %s" % (k, h(t), h(g[0]), h(g[1]), h(g[2])) for k, (t, g) in sorted(gyro.items())]
    path = str(tmp_path_factory.mktemp("pose") / "pose.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_estimated_gyro_mid_points_swap_interpolation_and_lowpass():
    res = frames()
    keys = sorted(res)
    plain = SY.estimated_gyro(res, FPS, 0.0, False)
    assert len(plain) == 10 and len(SY.estimated_gyro(res, FPS, 0.0, True)) == 11                     # the inner gap is interpolated, the trailing one has no neighbour
    k0, k1 = keys[0], keys[1]
    ts = k0 / 1000.0 + (k1 / 1000.0 - k0 / 1000.0) / 2.0
    t, g = plain[int(round(ts * 1000.0))]
    e = res[k0]
    assert t == ts and g == (e[1] * 180.0 / np.pi, e[0] * 180.0 / np.pi, e[2] * 180.0 / np.pi)
    full = SY.estimated_gyro(res, FPS, 0.0, True)
    ts4 = keys[4] / 1000.0 + (keys[5] / 1000.0 - keys[4] / 1000.0) / 2.0
    a, b = res[keys[3]], res[keys[5]]
    ratio = float(keys[4] - keys[3]) / float(keys[5] - keys[3])
    assert full[int(round(ts4 * 1000.0))][1][2] == (a[2] + (b[2] - a[2]) * ratio) * 180.0 / np.pi
    low = SY.estimated_gyro(res, FPS, 10.0, True)
    xyz, applied = warp.lowpass_gyro(10.0, FPS, np.array([full[k][1] for k in sorted(full)]))
    assert applied and [low[k][1] for k in sorted(low)] == [tuple(r) for r in xyz.tolist()]
    assert SY.estimated_gyro({}, FPS) == {}


def test_cpp_pose_host_half(exe, dump):
    out = subprocess.run([exe, "validate", dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok: 11 estimated samples of 12 frames" in out.stdout


@pytest.mark.gpu
def test_cpp_estimate_poses_almeida_on_the_device(exe, dump):
    out = subprocess.run([exe, "estimate", dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "estimate ok: 7 pairs" in out.stdout
