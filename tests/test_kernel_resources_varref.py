"""Register / LDS / scratch figures of the variational refinement's kernels (gyroflow_amd/csrc/gfw_varref.hip) against what DESIGN.md section 3.2l states, read from
the code objects inside libgfwarp.so (no GPU needed).  That the new unit moved no other kernel is tests/test_kernel_resources_dis.py's to hold (unchanged: five
kernels carry `gfw_dis_`, each at the figures of section 3.2k, and every earlier kernel at its recorded ones)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")
TAGS = ("gfw_varref_prepare_kernel", "gfw_varref_coeff_kernel", "gfw_varref_sor_kernel", "gfw_varref_apply_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgfwarp.so not built"
    return {k[".name"]: k for k in KR.report(LIB)}


def test_the_new_kernels_are_four_and_use_no_scratch_and_no_lds(kernels):
    new = sorted(n for n in kernels if "gfw_varref_" in n)
    assert len(new) == 4 and all(any(t in n for n in new) for t in TAGS), new
    assert not any("gfw_dis_" in n for n in new)
    for n in new:
        assert kernels[n][".private_segment_fixed_size"] == 0 and kernels[n][".group_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert not kernels[n].get(".uses_dynamic_stack", False), n
        assert kernels[n][".max_flat_workgroup_size"] == 256 and kernels[n].get(".wavefront_size", 64) == 64, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2l names each kernel with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for tag in TAGS:
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % re.escape(tag), text)
        assert m, "DESIGN.md does not state the figures of %s" % tag
        k = [v for n, v in kernels.items() if tag in n]
        assert len(k) == 1, tag
        got = (k[0][".vgpr_count"], k[0][".sgpr_count"], k[0][".group_segment_fixed_size"], k[0][".private_segment_fixed_size"])
        assert got == tuple(int(v) for v in m.groups()), (tag, got, m.groups())
    sor = [v for n, v in kernels.items() if "gfw_varref_sor_kernel" in n][0]
    assert sor[".vgpr_count"] <= 64                                          # the half-sweep, the hot path: eight waves a SIMD stay possible
