"""gyroflow::find_offsets_visual (include/gfwarp.hpp: the visual-features offset / readout-time search over gfw_sync_visual_search) driven by a C++ program
(tests/cpp/test_sync.cpp).  CPU: no ranges and the loud failure without a context.  GPU: ranges over a synthetic gyro track, against gfw_sync_visual_costs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_sync")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sync.cpp"), "-o", out,
                           "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def test_cpp_find_offsets_visual_validation(exe):
    out = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok" in out.stdout


@pytest.mark.gpu
def test_cpp_find_offsets_visual_on_the_device(exe):
    out = subprocess.run([exe, "search"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "search ok" in out.stdout
