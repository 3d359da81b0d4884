"""Register / LDS / scratch figures of the rs-sync offset search's kernels (gyroflow_amd/csrc/gfw_sync_rs.hip) against what DESIGN.md section 3.2n states, read from
the code objects inside libgfwarp.so (no GPU needed).  That every recorded kernel keeps its figures is tests/test_kernel_resources_record.py's to hold."""
from _kres import assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_rs_prepare_kernelILi1E", "gfw_rs_prepare_kernelILin1E", "gfw_rs_cost_kernel", "gfw_rs_pick_kernel")


def test_the_new_kernels_are_four_and_use_no_scratch(kernels):
    """no scratch, no spill, no dynamic stack, no accumulator registers; the cost stage is a one-wave workgroup under 128 registers (four waves a SIMD)"""
    new = sorted(n for n in kernels if "gfw_rs_" in n)
    assert len(new) == 4 and all(any(t in n for n in new) for t in TAGS), new
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".agpr_count"] == 0, n
        assert kernels[n][".max_flat_workgroup_size"] == (64 if "cost" in n else 256) and kernels[n][".vgpr_count"] <= 128, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2n names each kernel (the prepare stage's two instantiations as `gfw_rs_prepare_kernel<1>` and `<-1>`) with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    assert_design_md_figures(kernels, TAGS, {"gfw_rs_prepare_kernelILi1E": "gfw_rs_prepare_kernel<1>", "gfw_rs_prepare_kernelILin1E": "gfw_rs_prepare_kernel<-1>"})
    assert one(kernels, "gfw_rs_cost_kernel")[".group_segment_fixed_size"] == 0                   # m_i lives in dynamic LDS, 24 B a point of the call's largest pair
    lds = one(kernels, "gfw_rs_pick_kernel")[".group_segment_fixed_size"]
    assert 256 * 8 + 256 * 4 < lds <= 256 * 8 + 256 * 4 + 16                                    # a cost and an index a lane; the pick and its candidate
