"""Register / LDS / scratch figures of the essential-matrix pose estimation's kernels (gyroflow_amd/csrc/gfw_pose_essential.hip) against what DESIGN.md section 3.2m
states, read from the code objects inside libgfwarp.so (no GPU needed) — and every kernel that existed before that translation unit was added against the figures of
the build before it (tests/golden/kernel_resources_before_pose_essential.json, made from a build of the parent commit by the generator beside
tests/golden/kernel_resources_before_pose.json): the new unit moved none of them."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")
TAGS = ("gfw_pe_prepare_kernelILi1E", "gfw_pe_prepare_kernelILin1E", "gfw_pe_fit_kernel", "gfw_pe_count_kernel", "gfw_pe_pick_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgfwarp.so not built"
    return {k[".name"]: k for k in KR.report(LIB)}


def one(kernels, tag):
    hits = [k for n, k in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, len(hits))
    return hits[0]


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    """no scratch, no spill, no dynamic stack, no accumulator registers: the two kernels that hold a 9 x 9 eigenproblem per lane keep four rows of the eigenvector
    matrix in the lane's column of LDS, and everything else under 256 registers (two waves a SIMD)"""
    new = sorted(n for n in kernels if "gfw_pe_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    for n in new:
        assert kernels[n][".private_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert not kernels[n].get(".uses_dynamic_stack", False) and kernels[n][".agpr_count"] == 0, n
        assert kernels[n][".max_flat_workgroup_size"] == 256 and kernels[n][".vgpr_count"] <= 256, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2m names each kernel (the prepare stage's two instantiations as `gfw_pe_prepare_kernel<1>` and `<-1>`) with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    names = {"gfw_pe_prepare_kernelILi1E": "gfw_pe_prepare_kernel<1>", "gfw_pe_prepare_kernelILin1E": "gfw_pe_prepare_kernel<-1>"}
    for tag in TAGS:
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % re.escape(names.get(tag, tag)), text)
        assert m, "DESIGN.md does not state the figures of %s" % names.get(tag, tag)
        k = one(kernels, tag)
        got = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert got == tuple(int(v) for v in m.groups()), (tag, got, m.groups())
    rows = 4 * 9 * 256 * 8                                                                       # GFW_PE_LDS_ROWS rows of 9 doubles for each of 256 lanes
    assert one(kernels, "gfw_pe_fit_kernel")[".group_segment_fixed_size"] == rows                 # two workgroups a compute unit: the two waves a SIMD its registers allow
    assert one(kernels, "gfw_pe_count_kernel")[".group_segment_fixed_size"] == 0                  # counted by ballot
    # the pick stage: 256 (count, round), 4096 16-bit inlier indices, 45 x 64 f64 products, 45 sums, the pick, 4 x 4 front counts, and the eigenvector rows
    assert one(kernels, "gfw_pe_pick_kernel")[".group_segment_fixed_size"] == 256 * 8 + 4096 * 2 + 45 * 64 * 8 + 45 * 8 + 8 + 4 * 4 * 4 + rows


def test_every_kernel_that_existed_before_keeps_its_figures(kernels):
    """The fixture records ONE commit: the build before gfw_pose_essential.hip was added.  It shows that adding the unit moved no earlier kernel; it is not a budget for
    those kernels.  A later change that moves an earlier kernel ON PURPOSE regenerates the fixture from its parent's build or retires this test."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_pose_essential.json")))["kernels"]
    assert len(before) > 400
    missing = sorted(n for n in before if n not in kernels)
    assert not missing, missing[:5]
    fig = lambda k: [k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]]
    moved = {n: (fig(kernels[n]), want) for n, want in before.items() if fig(kernels[n]) != want}
    assert not moved, moved
    assert not any("gfw_pe_" in n for n in before)
