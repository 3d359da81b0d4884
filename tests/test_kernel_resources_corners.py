"""Register / LDS / scratch figures of the corner detection's kernels (gyroflow_amd/csrc/gfw_corners.hip) against what DESIGN.md section 3.2j states, read from the
code objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_corners_eig_kernel", "gfw_corners_pick_kernel", "gfw_corners_scan_kernel", "gfw_corners_pack_kernel")


def test_the_new_kernels_are_four_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_corners_" in n)
    assert len(new) == 4 and all(any(t in n for n in new) for t in TAGS), new
    assert not any("gfw_flow_" in n for n in new)                                                          # (tests/test_kernel_resources_flow.py counts those)
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".max_flat_workgroup_size"] == (64 if "gfw_corners_pack_kernel" in n else 256), n
        assert kernels[n].get(".wavefront_size", 64) == 64, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2j names each kernel with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS)
    # the haloed tile: 22 rows of 72 bytes, 20 x 68 derivative pairs, 18 x 66 scores, the maximum and four list bases
    assert one(kernels, "gfw_corners_eig_kernel")[".group_segment_fixed_size"] == 22 * 72 + 20 * 68 * 4 + 18 * 66 * 4 + 4 + 4 * 4
    assert one(kernels, "gfw_corners_pick_kernel")[".group_segment_fixed_size"] == 3 * 8                  # the ring of three 64-bit maxima
    assert one(kernels, "gfw_corners_scan_kernel")[".group_segment_fixed_size"] == 256 * 4
    assert one(kernels, "gfw_corners_eig_kernel")[".vgpr_count"] <= 64 and one(kernels, "gfw_corners_pick_kernel")[".vgpr_count"] <= 64      # eight waves a SIMD stay possible
