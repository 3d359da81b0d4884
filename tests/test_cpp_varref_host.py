"""gfw_flow_dis_refined's host code (gyroflow_amd/csrc/gfw_varref_host.h on top of gfw_dis_host.h: the check of the refinement's configuration, the two work
spaces under one limit, the plan, a level's argument block, the launch count of gfw_varref.h) in a stand-alone program (tests/cpp/test_varref_host.cpp) built with
AddressSanitizer and UBSan: the host pass of the project's compiler only, no device, no library, nothing loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "gyroflow_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc not found"
    out = str(tmp_path_factory.mktemp("cpp") / "test_varref_host")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "test_varref_host.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_varref_host_code_under_asan_and_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "varref host code ok" in r.stdout


def test_the_python_side_mirrors_the_headers():
    from gyroflow_amd import abi
    h = open(os.path.join(CSRC, "gfw_varref.h")).read()
    assert int(re.search(r"#define GFW_VARREF_ITERS_MAX (\d+)", h).group(1)) == abi.VARREF_ITERS_MAX
    planes = re.search(r"enum \{(.*?)GFW_VARREF_PLANES \};", h, re.S).group(1)
    assert len(re.findall(r"GFW_VR_\w+", planes)) == abi.VARREF_PLANES
    assert C.sizeof(abi.FlowVarrefCfg) == 32 and abi.FlowVarrefCfg.omega.offset == 20
    d = abi.varref_cfg()
    assert (d.fixed_point_iters, d.sor_iters, d.alpha, d.delta, d.gamma, round(d.omega, 6), list(d.reserved)) == (5, 5, 20.0, 5.0, 10.0, 1.6, [0, 0])
    assert "gfw_flow_dis_refined" in abi.EXPORTS
    # the one translation unit of the refinement is in the build list, and its kernels never carry the DIS kernels' tag
    assert 'add(os.path.join(CSRC, "gfw_varref.hip")' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    names = re.findall(r"__global__[^\n]*?void (\w+)\(", open(os.path.join(CSRC, "gfw_varref.hip")).read())
    assert sorted(names) == ["gfw_varref_apply_kernel", "gfw_varref_coeff_kernel", "gfw_varref_prepare_kernel", "gfw_varref_sor_kernel"]
