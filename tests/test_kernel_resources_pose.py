"""Register / LDS / scratch figures of the pose estimation's kernels (gyroflow_amd/csrc/gfw_pose.hip) against what DESIGN.md section 3.2h states, read from the code
objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_pose_prepare_kernelILi1E", "gfw_pose_prepare_kernelILin1E", "gfw_pose_fit_kernel", "gfw_pose_count_kernel", "gfw_pose_pick_kernel")


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_pose_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".max_flat_workgroup_size"] == 256


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2h names each kernel (the prepare stage's two instantiations as `gfw_pose_prepare_kernel<1>` and `<-1>`) with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS, {"gfw_pose_prepare_kernelILi1E": "gfw_pose_prepare_kernel<1>", "gfw_pose_prepare_kernelILin1E": "gfw_pose_prepare_kernel<-1>"})
    assert one(kernels, "gfw_pose_fit_kernel")[".group_segment_fixed_size"] == 0                       # 30 dependent steps on 3 points in registers: no LDS
    assert one(kernels, "gfw_pose_count_kernel")[".group_segment_fixed_size"] == 0                     # counted by ballot
    # the pick stage: 256 (count, round), 4096 16-bit inlier indices, 6 x 256 products, 6 sums, the pick
    assert one(kernels, "gfw_pose_pick_kernel")[".group_segment_fixed_size"] == 256 * 8 + 4096 * 2 + 6 * 256 * 4 + 6 * 4 + 8
