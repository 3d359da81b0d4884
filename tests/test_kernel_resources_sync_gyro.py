"""Register / LDS / scratch figures of the gyro-match search's kernels (gyroflow_amd/csrc/gfw_sync_gyro.hip) against what DESIGN.md section 3.2f states, read from the
code objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import KR, assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)


def test_the_new_kernels_are_two_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_gyro_" in n)
    assert len(new) == 2 and "cost" in new[0] and "pick" in new[1], new
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".max_flat_workgroup_size"] == 256


def test_the_figures_design_md_states(kernels):
    """`gfw_gyro_cost_kernel` 18 VGPR / 46 SGPR / no LDS, `gfw_gyro_pick_kernel` 12 VGPR / 32 SGPR / 3080 B LDS (256 x (f64 cost, index), the pick)"""
    assert_design_md_figures(kernels, ("gfw_gyro_cost_kernel", "gfw_gyro_pick_kernel"))
    assert one(kernels, "gfw_gyro_cost_kernel")[".group_segment_fixed_size"] == 0
    assert KR.waves_per_simd(one(kernels, "gfw_gyro_cost_kernel")[".vgpr_count"]) == 8              # a lane is a candidate: every wave a SIMD can hold
