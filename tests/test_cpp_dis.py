"""gyroflow::optical_flow_dis (include/gfwarp.hpp: the DIS dense flow over gfw_flow_dis) driven by a C++ program (tests/cpp/test_dis.cpp) against a dump of the
numpy statement's results (tests/_disstmt.py).  CPU: no pairs, and the loud failure without a context.  GPU: every pair's points equal to the statement's to the
bit, at the reference's finest scale and at 1."""
import os
import subprocess

import pytest

import _discase as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_dis")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_dis.cpp"), "-o", out, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


def pair_lines(s):
    lines = []
    first = s["pair_first"]
    for p in range(len(first) - 1):
        a, b = s["points_a"][first[p]:first[p + 1]], s["points_b"][first[p]:first[p + 1]]
        lines.append("%d %d" % ((1, len(a)) if len(a) >= 10 else (0, 0)))
        if len(a) >= 10:
            lines += ["%s %s %s %s" % (h(x[0]), h(x[1]), h(y[0]), h(y[1])) for x, y in zip(a, b)]
    return lines


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    name = "cut-200x168"
    c = DC.case(name)
    lines = [bytes(c.cam.kp).hex(), "%d %d" % (c.cam.clip.model, c.cam.clip.digital), "3 %d %d %d" % (c.width, c.height, c.stride), str(len(c.pairs))]
    lines += ["%d %d" % p for p in c.pairs]
    lines += pair_lines(DC.statement(name, 2)[0]) + pair_lines(DC.statement(name, 1)[0])
    d = tmp_path_factory.mktemp("dis")
    path, frames = str(d / "dis.txt"), str(d / "frames.bin")
    open(path, "w").write("\n".join(lines) + "\n")
    c.frames.tofile(frames)
    return path, frames


def test_cpp_dis_without_a_context(exe, dump):
    r = subprocess.run([exe, "validate", *dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "validate ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_dis_on_the_device_equals_the_statement(exe, dump):
    r = subprocess.run([exe, "flow", *dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "flow ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
