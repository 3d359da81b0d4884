"""The host code the point-pair calls share (gyroflow_amd/csrc/gfw_pairs_host.h: the pair-set check, the staged firsts and points in both base modes, the lens
gate) and the visual search's check (gfw_sync_check, gfw_sync_host.h) in a stand-alone program (tests/cpp/test_pairs_host.cpp) built with AddressSanitizer and
UBSan: the host pass of the project's compiler only, no device, no library, nothing loaded into Python.  The program holds the refusals to their texts and the staged
parts to their bytes; the sanitizers hold every access."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc not found"
    out = str(tmp_path_factory.mktemp("cpp") / "test_pairs_host")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "test_pairs_host.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_pairs_host_code_under_asan_and_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pairs host code ok" in r.stdout
