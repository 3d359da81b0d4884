"""gyroflow::detect_features_pyrlk (include/gfwarp.hpp: Shi-Tomasi corner detection over gfw_corners_shi_tomasi) driven by a C++ program (tests/cpp/test_corners.cpp)
against a dump of the numpy statement's results (tests/_cornerstmt.py).  CPU: no frames, and the loud failure without a context.  GPU: every frame's corners equal
to the statement's to the bit, and gyroflow::optical_flow_pyrlk on them gives the kept points of the CPU chain (tests/_cornercase.chain)."""
import os
import subprocess

import pytest

import _cornercase as CC
import _flowcase as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")
NAME = "cut-200x168"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_corners")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_corners.cpp"), "-o", out, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    c, cam = CC.case(NAME), FC.case(NAME).cam
    feats, _ = CC.chain(NAME)
    lines = [bytes(cam.kp).hex(), "%d %d" % (cam.clip.model, cam.clip.digital), "3 %d %d %d" % (c.width, c.height, c.stride)]
    for f in feats:
        lines.append(str(len(f)))
        lines += ["%s %s" % (h(x), h(y)) for x, y in f]
    lines.append(str(len(FC.PAIRS)))
    lines += ["%d %d" % p for p in FC.PAIRS]
    for a, b in CC.chain_pairs(NAME):
        assert len(a) >= 10
        lines.append("1 %d" % len(a))
        lines += ["%s %s %s %s" % (h(x[0]), h(x[1]), h(y[0]), h(y[1])) for x, y in zip(a, b)]
    d = tmp_path_factory.mktemp("corners")
    path, frames = str(d / "corners.txt"), str(d / "frames.bin")
    open(path, "w").write("\n".join(lines) + "\n")
    c.frames.tofile(frames)
    return path, frames


def test_cpp_corners_without_a_context(exe, dump):
    r = subprocess.run([exe, "validate", *dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "validate ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_corners_on_the_device_equal_the_statement(exe, dump):
    r = subprocess.run([exe, "detect", *dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "detect ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
