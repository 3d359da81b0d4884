"""The gyroflow::calculate_fovs overload that takes per-frame stabiliser data and meshes (include/gfwarp.hpp, over gfw_zoom_fovs_stab + gfw_zoom_smooth)
driven by a C++ program (tests/cpp/test_zoom_stab.cpp).  CPU: the empty clip, tables of the wrong length, the loud failure without a context.  GPU: a clip
with caller-given rotations, IBIS splines on the even frames and two shared meshes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")):
        pytest.skip("libgfwarp.so not built")
    out = str(tmp_path_factory.mktemp("cpp") / "test_zoom_stab")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_zoom_stab.cpp"), "-o", out,
                           "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def test_cpp_calculate_fovs_validation(exe):
    out = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok" in out.stdout


@pytest.mark.gpu
def test_cpp_calculate_fovs_on_the_device(exe):
    out = subprocess.run([exe, "fovs"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fovs ok" in out.stdout
