"""gyroflow::optical_flow_pyrlk (include/gfwarp.hpp: pyramidal Lucas-Kanade optical flow over gfw_flow_pyrlk) driven by a C++ program (tests/cpp/test_flow.cpp)
against a dump of the numpy statement's results (tests/_flowstmt.py).  CPU: no pairs, and the loud failure without a context.  GPU: every pair's kept points equal
to the statement's to the bit, with the caller's features and with the grid points."""
import os
import subprocess

import pytest

import _flowcase as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_flow")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_flow.cpp"), "-o", out, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


def kept_lines(s):
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
    c = FC.case("cut-200x168")
    feats = [f[:16] for f in c.features]                                  # (finite features only: the dump is text)
    import _flowstmt as FS
    want = FS.flow_pyrlk(c.frames[:, :, :c.width], FC.PAIRS, feats)
    lines = [bytes(c.cam.kp).hex(), "%d %d" % (c.cam.clip.model, c.cam.clip.digital), "3 %d %d %d" % (c.width, c.height, c.stride), str(len(FC.PAIRS))]
    lines += ["%d %d" % p for p in FC.PAIRS]
    for f in feats:
        lines.append(str(len(f)))
        lines += ["%s %s" % (h(x), h(y)) for x, y in f]
    lines += kept_lines(want) + kept_lines(c.grid_statement)
    d = tmp_path_factory.mktemp("flow")
    path, frames = str(d / "flow.txt"), str(d / "frames.bin")
    open(path, "w").write("\n".join(lines) + "\n")
    c.frames.tofile(frames)
    return path, frames


def test_cpp_flow_without_a_context(exe, dump):
    r = subprocess.run([exe, "validate", *dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "validate ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_flow_on_the_device_equals_the_statement(exe, dump):
    r = subprocess.run([exe, "track", *dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "track ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
