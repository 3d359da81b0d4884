"""Register / LDS / scratch figures of the DIS dense flow's kernels (gyroflow_amd/csrc/gfw_dis.hip) against what DESIGN.md section 3.2k states, read from the code
objects inside libgfwarp.so (no GPU needed) — and every kernel that existed before that translation unit was added against the figures of the build before it
(tests/golden/kernel_resources_before_dis.json): the new unit moved none of them."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")
TAGS = ("gfw_dis_pyramid_kernel", "gfw_dis_pass_kernel", "gfw_dis_dense_kernel", "gfw_dis_scan_kernel", "gfw_dis_nodes_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgfwarp.so not built"
    return {k[".name"]: k for k in KR.report(LIB)}


def one(kernels, tag):
    hits = [k for n, k in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, len(hits))
    return hits[0]


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_dis_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    for n in new:
        assert kernels[n][".private_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert not kernels[n].get(".uses_dynamic_stack", False), n
        assert kernels[n][".max_flat_workgroup_size"] == (64 if "gfw_dis_pass_kernel" in n or "gfw_dis_nodes_kernel" in n else 256), n
        assert kernels[n].get(".wavefront_size", 64) == 64, n


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2k names each kernel with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for tag in TAGS:
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % re.escape(tag), text)
        assert m, "DESIGN.md does not state the figures of %s" % tag
        k = one(kernels, tag)
        got = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert got == tuple(int(v) for v in m.groups()), (tag, got, m.groups())
    assert one(kernels, "gfw_dis_pass_kernel")[".group_segment_fixed_size"] == 3 * 5 * 8                  # the ring of three rows of five 64-bit sums
    assert one(kernels, "gfw_dis_scan_kernel")[".group_segment_fixed_size"] == 256 * 4
    assert one(kernels, "gfw_dis_pass_kernel")[".vgpr_count"] <= 64                                     # eight waves a SIMD stay possible


def test_every_kernel_that_existed_before_keeps_its_figures(kernels):
    """The fixture records ONE commit: the build before gfw_dis.hip was added (tests/golden/kernel_resources_before_dis.py makes it).  It shows that adding the unit
    moved no earlier kernel; it is not a budget for those kernels.  A later change that moves an earlier kernel ON PURPOSE regenerates the fixture from its parent's
    build or retires this test."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_dis.json")))["kernels"]
    assert len(before) > 300
    missing = sorted(n for n in before if n not in kernels)
    assert not missing, missing[:5]
    fig = lambda k: [k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]]
    moved = {n: (fig(kernels[n]), want) for n, want in before.items() if fig(kernels[n]) != want}
    assert not moved, moved
    assert not any("gfw_dis_" in n for n in before) and any("gfw_corners_" in n for n in before)
