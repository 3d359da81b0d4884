"""gfw_pose_almeida's host code (gyroflow_amd/csrc/gfw_pose_host.h: the check that names the pair, the staging, the call's constants) and gfw_pose_draws' generator in
a stand-alone program (tests/cpp/test_pose_host.cpp) built with AddressSanitizer and UBSan: the host pass of the project's compiler only, no device, no library,
nothing loaded into Python.  The program holds the draws to their contract — indices in range, distinct within a triple, every list a permutation prefix, a function
of the seed — and the staged block to its layout; the sanitizers hold every access."""
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
    out = str(tmp_path_factory.mktemp("cpp") / "test_pose_host")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "test_pose_host.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_pose_host_code_under_asan_and_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pose host code ok" in r.stdout


def test_the_librarys_draws_are_in_range_distinct_and_permutation_prefixes():
    """warp.pose_draws (gfw_pose_draws of the built library): the same contract seen from Python"""
    counts = [0, 1, 2, 3, 12, 65, 200]
    for num_samples in (40, 1000):
        triples, samples = warp.pose_draws(5, counts, 9, num_samples)
        assert triples.shape == (len(counts), 9, 3)
        for p, n in enumerate(counts):
            m = min(n, num_samples)
            assert samples[p].shape == (9, m)
            if n < 3:
                assert not triples[p].any()
                continue
            assert triples[p].min() >= 0 and triples[p].max() < n and all(len(set(t)) == 3 for t in triples[p].tolist())
            assert samples[p].min() >= 0 and samples[p].max() < n and all(len(set(s)) == m for s in samples[p].tolist())
        assert len({tuple(s) for s in samples[5].tolist()}) == 9                                     # rounds differ
    again, _ = warp.pose_draws(5, counts, 9, 40)
    other, _ = warp.pose_draws(6, counts, 9, 40)
    assert np.array_equal(again, warp.pose_draws(5, counts, 9, 1000, lists=False)[0]) and not np.array_equal(again, other)
