"""Register / LDS / scratch budget of the sync search's kernels (gyroflow_amd/csrc/gfw_sync.hip), read from the code objects inside libgfwarp.so (no GPU needed).

A (candidate, pair) of the cost stage is ONE wave: how many of them a CU holds at once is what hides the f64 slerp's latency, so the wave's registers are pinned at
what the build gives, none of the three kernels may spill, and the cost kernel's LDS is the call's largest pair (asked for at launch, up to 16 KB) plus a fixed
part that stays small."""
import pytest

from _kres import KR, load, one


@pytest.fixture(scope="module")
def kernels():
    ks = {n: k for n, k in load().items() if "gfw_sync_" in n}
    assert len(ks) == 4, sorted(ks)                  # the lens stage for the fisheye and the generic model, the cost stage, the reduce stage
    return ks


def test_no_scratch(kernels):
    for n, k in kernels.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])


def test_cost_kernel(kernels):
    k = one(kernels, "gfw_sync_cost_kernel")
    assert k[".vgpr_count"] <= 111 and k[".sgpr_count"] <= 106, (k[".vgpr_count"], k[".sgpr_count"])            # four waves per SIMD
    assert KR.waves_per_simd(k[".vgpr_count"]) >= 4
    assert k[".group_segment_fixed_size"] <= 160, k[".group_segment_fixed_size"]    # two rotations, two prefixes + start times, the sum; the distances are asked for at launch: 4 B x the largest pair, at most 4096 points = 16 KB
    assert k[".max_flat_workgroup_size"] == 64


def test_lens_and_reduce_kernels(kernels):
    for tag, vgpr, sgpr in (("gfw_sync_rays_kernelILi1E", 19, 30), ("gfw_sync_rays_kernelILin1E", 26, 49), ("gfw_sync_reduce_kernel", 14, 30)):
        k = one(kernels, tag)
        assert k[".vgpr_count"] <= vgpr and k[".sgpr_count"] <= sgpr, (tag, k[".vgpr_count"], k[".sgpr_count"])
    assert one(kernels, "gfw_sync_rays_kernelILi1E")[".group_segment_fixed_size"] == 0
    assert one(kernels, "gfw_sync_reduce_kernel")[".group_segment_fixed_size"] <= 3080            # 256 x (f64 cost, index), the pick
