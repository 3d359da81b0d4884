"""Register / LDS / scratch figures of the sync-point choice's kernels (gyroflow_amd/csrc/gfw_sync_optim.hip) against what DESIGN.md section 3.2g states, read from
the code objects inside libgfwarp.so (no GPU needed): no scratch, no spills, and the documented numbers."""
from _kres import KR, assert_design_md_figures, assert_no_scratch, kernels, one          # noqa: F401 (kernels: the fixture)

TAGS = ("gfw_optim_spectrum_kernel", "gfw_optim_max_kernel", "gfw_optim_rank_kernel", "gfw_optim_nms_kernel", "gfw_optim_pick_kernel", "gfw_optim_gather_kernel")


def test_the_new_kernels_are_six_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_optim_" in n)
    assert len(new) == 6 and all(any(t in n for n in new) for t in TAGS), new
    assert not any("gfw_gyro_" in n for n in new)
    assert_no_scratch(kernels, new)
    for n in new:
        assert kernels[n][".max_flat_workgroup_size"] == 256


def test_the_figures_design_md_states(kernels):
    assert_design_md_figures(kernels, TAGS)
    spectrum = one(kernels, "gfw_optim_spectrum_kernel")
    assert spectrum[".group_segment_fixed_size"] == 257 * 6 * 4 + 8 or spectrum[".group_segment_fixed_size"] == 257 * 6 * 4      # the round's bins (+ the dynamic part's alignment)
    assert KR.waves_per_simd(spectrum[".vgpr_count"]) == 8                                # registers do not limit the waves a SIMD holds: LDS does, at 18 N bytes a workgroup
    # the static part and the largest dynamic part fit the 160 KB of a gfx950 compute unit
    assert spectrum[".group_segment_fixed_size"] + 18 * 8192 <= 160 * 1024
