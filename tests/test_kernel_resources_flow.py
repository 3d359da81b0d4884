"""Register / LDS / scratch figures of the optical flow's kernels (gyroflow_amd/csrc/gfw_flow.hip) against what DESIGN.md section 3.2i states, read from the code
objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_flow_pyramid_kernel", "gfw_flow_grid_kernel", "gfw_flow_track_kernel", "gfw_flow_scan_kernel", "gfw_flow_compact_kernel")
WAVE_KERNELS = ("gfw_flow_grid_kernel", "gfw_flow_track_kernel", "gfw_flow_compact_kernel")      # a workgroup is one wave: a barrier is a wave barrier


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_flow_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".max_flat_workgroup_size"] == (64 if any(t in n for t in WAVE_KERNELS) else 256), n
        assert kernels[n].get(".wavefront_size", 64) == 64, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2i names each kernel with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS)
    assert one(kernels, "gfw_flow_track_kernel")[".group_segment_fixed_size"] == 3 * 3 * 8                # the ring of three accumulators of three 64-bit sums
    assert one(kernels, "gfw_flow_scan_kernel")[".group_segment_fixed_size"] == 256 * 4
    assert one(kernels, "gfw_flow_track_kernel")[".vgpr_count"] <= 128                                     # the 441-pixel template in registers (21 of them) without a spill; what that costs in occupancy is not measured
