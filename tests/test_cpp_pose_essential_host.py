"""gfw_pose_essential's host code (gyroflow_amd/csrc/gfw_pose_essential_host.h: the check that names the pair, the staging, the call's constants) and
gfw_pose_draws_k's generator (gfw_pose_host.h) in a stand-alone program (tests/cpp/test_pose_essential_host.cpp) built with AddressSanitizer and UBSan: the host
pass of the project's compiler only, no device, no library, nothing loaded into Python.  The program holds the draws to their contract — indices in range, distinct
within a tuple, a function of the seed, k = 3 equal to gfw_pose_draws' triples — and the staged block to its layout; the sanitizers hold every access."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gyroflow_amd import warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc not found"
    out = str(tmp_path_factory.mktemp("cpp") / "test_pose_essential_host")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "test_pose_essential_host.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_pose_essential_host_code_under_asan_and_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pose essential host code ok" in r.stdout


def test_the_librarys_draws_are_in_range_distinct_and_a_function_of_the_seed():
    """warp.pose_draws_k (gfw_pose_draws_k of the built library): the same contract seen from Python"""
    counts = [0, 7, 8, 9, 65, 200]
    octets = warp.pose_draws_k(5, counts, 9, 8)
    assert octets.shape == (len(counts), 9, 8) and octets.dtype == np.int32
    for p, n in enumerate(counts):
        if n < 8:
            assert not octets[p].any()
            continue
        assert octets[p].min() >= 0 and octets[p].max() < n and all(len(set(o)) == 8 for o in octets[p].tolist())
    assert len({tuple(o) for o in octets[4].tolist()}) == 9                                          # rounds differ
    assert np.array_equal(octets, warp.pose_draws_k(5, counts, 9, 8)) and not np.array_equal(octets, warp.pose_draws_k(6, counts, 9, 8))
    assert np.array_equal(warp.pose_draws_k(5, counts, 9, 3), warp.pose_draws(5, counts, 9, 1000, lists=False)[0])      # k = 3: gfw_pose_draws' triples
    with pytest.raises(warp.GfwError):
        warp.pose_draws_k(5, counts, 9, 17)
