"""Register / LDS / scratch figures of the DIS dense flow's kernels (gyroflow_amd/csrc/gfw_dis.hip) against what DESIGN.md section 3.2k states, read from the code
objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_dis_pyramid_kernel", "gfw_dis_pass_kernel", "gfw_dis_dense_kernel", "gfw_dis_scan_kernel", "gfw_dis_nodes_kernel")


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_dis_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".max_flat_workgroup_size"] == (64 if "gfw_dis_pass_kernel" in n or "gfw_dis_nodes_kernel" in n else 256), n
        assert kernels[n].get(".wavefront_size", 64) == 64, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2k names each kernel with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS)
    assert one(kernels, "gfw_dis_pass_kernel")[".group_segment_fixed_size"] == 3 * 5 * 8                  # the ring of three rows of five 64-bit sums
    assert one(kernels, "gfw_dis_scan_kernel")[".group_segment_fixed_size"] == 256 * 4
    assert one(kernels, "gfw_dis_pass_kernel")[".vgpr_count"] <= 64                                     # eight waves a SIMD stay possible
