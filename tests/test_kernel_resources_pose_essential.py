"""Register / LDS / scratch figures of the essential-matrix pose estimation's kernels (gyroflow_amd/csrc/gfw_pose_essential.hip) against what DESIGN.md section 3.2m
states, read from the code objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to
hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_pe_prepare_kernelILi1E", "gfw_pe_prepare_kernelILin1E", "gfw_pe_fit_kernel", "gfw_pe_count_kernel", "gfw_pe_pick_kernel")


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    """no scratch, no spill, no dynamic stack, no accumulator registers: the two kernels that hold a 9 x 9 eigenproblem per lane keep four rows of the eigenvector
    matrix in the lane's column of LDS, and everything else under 256 registers (two waves a SIMD)"""
    new = sorted(n for n in kernels if "gfw_pe_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".agpr_count"] == 0, n
        assert kernels[n][".max_flat_workgroup_size"] == 256 and kernels[n][".vgpr_count"] <= 256, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2m names each kernel (the prepare stage's two instantiations as `gfw_pe_prepare_kernel<1>` and `<-1>`) with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS, {"gfw_pe_prepare_kernelILi1E": "gfw_pe_prepare_kernel<1>", "gfw_pe_prepare_kernelILin1E": "gfw_pe_prepare_kernel<-1>"})
    rows = 4 * 9 * 256 * 8                                                                       # GFW_PE_LDS_ROWS rows of 9 doubles for each of 256 lanes
    assert one(kernels, "gfw_pe_fit_kernel")[".group_segment_fixed_size"] == rows                 # two workgroups a compute unit: the two waves a SIMD its registers allow
    assert one(kernels, "gfw_pe_count_kernel")[".group_segment_fixed_size"] == 0                  # counted by ballot
    # the pick stage: 256 (count, round), 4096 16-bit inlier indices, 45 x 64 f64 products, 45 sums, the pick, 4 x 4 front counts, and the eigenvector rows
    assert one(kernels, "gfw_pe_pick_kernel")[".group_segment_fixed_size"] == 256 * 8 + 4096 * 2 + 45 * 64 * 8 + 45 * 8 + 8 + 4 * 4 * 4 + rows
