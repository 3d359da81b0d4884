"""gfw_flow_dis's host code (gyroflow_amd/csrc/gfw_dis_host.h: the check that names the pair or frame, the coarsest scale and the level sizes, the plan and the
staging) in a stand-alone program (tests/cpp/test_dis_host.cpp) built with AddressSanitizer and UBSan: the host pass of the project's compiler only, no device, no
library, nothing loaded into Python.  The program holds the staged block to its plan; the sanitizers hold every access."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc not found"
    out = str(tmp_path_factory.mktemp("cpp") / "test_dis_host")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "test_dis_host.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_dis_host_code_under_asan_and_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "dis host code ok" in r.stdout


def test_the_python_side_limits_are_the_host_codes():
    """abi.DIS_RING_SLOTS is what tests/test_gpu_dis.py sizes its 'one call more than the ring has slots' by: it must be gfw_ctx::kDisSlots; the limits are gfw_dis.h's"""
    import re
    from gyroflow_amd import abi
    m = re.search(r"kDisSlots = (\d+);", open(os.path.join(ROOT, "gyroflow_amd", "csrc", "gfw_api.hip")).read())
    assert m and int(m.group(1)) == abi.DIS_RING_SLOTS
    h = open(os.path.join(ROOT, "gyroflow_amd", "csrc", "gfw_dis.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, h).group(1))
    assert (define("GFW_DIS_NODES_MAX"), define("GFW_DIS_PAIRS_MAX"), define("GFW_DIS_FRAMES_MAX"), define("GFW_DIS_SIDE_MAX")) == \
        (abi.DIS_NODES_MAX, abi.DIS_PAIRS_MAX, abi.DIS_FRAMES_MAX, abi.DIS_SIDE_MAX)
    import ctypes as C
    assert C.sizeof(abi.FlowDisCfg) == 24
