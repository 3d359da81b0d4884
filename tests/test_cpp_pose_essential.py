"""gyroflow::estimate_poses_essential (include/gfwarp.hpp: essential-matrix pose estimation over gfw_pose_essential) driven by a C++ program
(tests/cpp/test_pose_essential.cpp) against a dump of the numpy statement's results (tests/_posessstmt.py) under the library's own draws (gfw_pose_draws_k: host
code).  CPU: pairs without points, the loud failure without a context.  GPU: quaternions, rotations, essential matrices and best rounds equal to the statement's to
the bit; euler within 1e-12 (the same f64 formula through two math libraries' acos); pairs without a rotation come back without one."""
import os
import subprocess

import numpy as np
import pytest

from gyroflow_amd import synchronization as SY, warp
import _posesscase as EC
import _posessstmt as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")
SEED, FPS, NTH = 20241, 59.94, 2.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_pose_essential")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pose_essential.cpp"), "-o", out, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


def stated_pairs():
    """pairs of the fisheye case (None in front and inside; 7, 8 and 9 points: no rotation), and what the statement makes of them under the library's draws for SEED"""
    c = EC.case("fisheye-r7")
    pairs = [None] + list(c.pairs[1:5]) + [None] + list(c.pairs[5:7])
    live = [p for p in pairs if p is not None]
    octets = warp.pose_draws_k(SEED, [len(a) for a, _ in live], c.cam.num_iters, 8)
    quats, rot, ess, best, _, _ = ES.estimate(c.cam, live, octets)
    want, k = [], 0
    for p in pairs:
        if p is None:
            want.append(None)
        else:
            want.append(dict(quat=quats[k], rotation=rot[k], essential=ess[k], best=best[k], euler=SY.scaled_axis(rot[k]) * (FPS / NTH)))
            k += 1
    return c, pairs, want


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    c, pairs, want = stated_pairs()
    cam = c.cam
    cfg = EC.cfg_of(cam)
    lines = [bytes(cam.kp).hex(), "%d %d" % (cam.clip.model, cam.clip.digital),
             "%d %d %d %d %d %d %s %s" % (cfg.video_width, cfg.video_height, cfg.flow_width, cfg.flow_height, cfg.num_iters, cfg.min_front, h(cfg.inlier_threshold),
                                          " ".join(h(cfg.camera_matrix[i]) for i in range(9))),
             "%s %s %d" % (h(FPS), h(NTH), SEED), str(len(pairs))]
    ident = [1.0, 0.0, 0.0, 0.0] + [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] + [0.0] * 12
    for p, w in zip(pairs, want):
        if p is None:
            lines += ["0 0", "0 " + " ".join(h(v) for v in ident) + " 0 -1 0"]
            continue
        a, b = p
        lines.append("1 %d" % len(a))
        lines += ["%s %s %s %s" % (h(x[0]), h(x[1]), h(y[0]), h(y[1])) for x, y in zip(a, b)]
        lines.append("%d " % w["best"][3] + " ".join(h(v) for v in list(w["quat"]) + list(w["rotation"].reshape(9)) + list(w["essential"]) + list(w["euler"]))
                     + " %d %d %d" % tuple(w["best"][:3]))
    path = str(tmp_path_factory.mktemp("pose") / "pose_essential.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_the_dumped_pairs_have_and_lack_rotations():
    _, pairs, want = stated_pairs()
    found = [w["best"][3] for w in want if w is not None]
    assert 0 in found and 1 in found and len(pairs) == 8


def test_cpp_pose_essential_host_half(exe, dump):
    out = subprocess.run([exe, "validate", dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok: 8 pairs" in out.stdout


@pytest.mark.gpu
def test_cpp_estimate_poses_essential_on_the_device(exe, dump):
    out = subprocess.run([exe, "estimate", dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "estimate ok: 8 pairs" in out.stdout
