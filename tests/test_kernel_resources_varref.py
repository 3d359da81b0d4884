"""Register / LDS / scratch figures of the variational refinement's kernels (gyroflow_amd/csrc/gfw_varref.hip) against what DESIGN.md section 3.2l states, read from
the code objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_varref_prepare_kernel", "gfw_varref_coeff_kernel", "gfw_varref_sor_kernel", "gfw_varref_apply_kernel")


def test_the_new_kernels_are_four_and_use_no_scratch_and_no_lds(kernels):
    new = sorted(n for n in kernels if "gfw_varref_" in n)
    assert len(new) == 4 and all(any(t in n for n in new) for t in TAGS), new
    assert not any("gfw_dis_" in n for n in new)
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".group_segment_fixed_size"] == 0, n
        assert kernels[n][".max_flat_workgroup_size"] == 256 and kernels[n].get(".wavefront_size", 64) == 64, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2l names each kernel with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS)
    assert one(kernels, "gfw_varref_sor_kernel")[".vgpr_count"] <= 64       # the half-sweep, the hot path: eight waves a SIMD stay possible
