"""Register / LDS / scratch figures of the pose estimation's kernels (gyroflow_amd/csrc/gfw_pose.hip) against what DESIGN.md section 3.2h states, read from the code
objects inside libgfwarp.so (no GPU needed) — and every kernel that existed before that translation unit was added against the figures of the build before it
(tests/golden/kernel_resources_before_pose.json): the new unit moved none of them."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")
TAGS = ("gfw_pose_prepare_kernelILi1E", "gfw_pose_prepare_kernelILin1E", "gfw_pose_fit_kernel", "gfw_pose_count_kernel", "gfw_pose_pick_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgfwarp.so not built"
    return {k[".name"]: k for k in KR.report(LIB)}


def one(kernels, tag):
    hits = [k for n, k in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, len(hits))
    return hits[0]


def test_the_new_kernels_are_five_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_pose_" in n)
    assert len(new) == 5 and all(any(t in n for n in new) for t in TAGS), new
    for n in new:
        assert kernels[n][".private_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert not kernels[n].get(".uses_dynamic_stack", False), n
        assert kernels[n][".max_flat_workgroup_size"] == 256


def test_the_figures_design_md_states(kernels):
    """DESIGN.md 3.2h names each kernel (the prepare stage's two instantiations as `gfw_pose_prepare_kernel<1>` and `<-1>`) with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    names = {"gfw_pose_prepare_kernelILi1E": "gfw_pose_prepare_kernel<1>", "gfw_pose_prepare_kernelILin1E": "gfw_pose_prepare_kernel<-1>"}
    for tag in TAGS:
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % re.escape(names.get(tag, tag)), text)
        assert m, "DESIGN.md does not state the figures of %s" % names.get(tag, tag)
        k = one(kernels, tag)
        got = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert got == tuple(int(v) for v in m.groups()), (tag, got, m.groups())
    assert one(kernels, "gfw_pose_fit_kernel")[".group_segment_fixed_size"] == 0                       # 30 dependent steps on 3 points in registers: no LDS
    assert one(kernels, "gfw_pose_count_kernel")[".group_segment_fixed_size"] == 0                     # counted by ballot
    # the pick stage: 256 (count, round), 4096 16-bit inlier indices, 6 x 256 products, 6 sums, the pick
    assert one(kernels, "gfw_pose_pick_kernel")[".group_segment_fixed_size"] == 256 * 8 + 4096 * 2 + 6 * 256 * 4 + 6 * 4 + 8


def test_every_kernel_that_existed_before_keeps_its_figures(kernels):
    """The fixture records ONE commit: the build before gfw_pose.hip was added (tests/golden/kernel_resources_before_pose.py makes it).  It shows that adding the unit
    moved no earlier kernel; it is not a budget for those kernels.  A later change that moves an earlier kernel ON PURPOSE regenerates the fixture from its parent's
    build or retires this test."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_pose.json")))["kernels"]
    assert len(before) > 300
    missing = sorted(n for n in before if n not in kernels)
    assert not missing, missing[:5]
    fig = lambda k: [k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]]
    moved = {n: (fig(kernels[n]), want) for n, want in before.items() if fig(kernels[n]) != want}
    assert not moved, moved
    assert not any("gfw_pose_" in n for n in before)
