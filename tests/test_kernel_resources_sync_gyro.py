"""Register / LDS / scratch figures of the gyro-match search's kernels (gyroflow_amd/csrc/gfw_sync_gyro.hip) against what DESIGN.md section 3.2f states, read from the
code objects inside libgfwarp.so (no GPU needed) — and every kernel that existed before that translation unit was added against the figures of the build before it
(tests/golden/kernel_resources_before_sync_gyro.json): the new unit moved none of them."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgfwarp.so not built"
    return {k[".name"]: k for k in KR.report(LIB)}


def one(kernels, tag):
    hits = [k for n, k in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, len(hits))
    return hits[0]


def test_the_new_kernels_are_two_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_gyro_" in n)
    assert len(new) == 2 and "cost" in new[0] and "pick" in new[1], new
    for n in new:
        assert kernels[n][".private_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert kernels[n][".max_flat_workgroup_size"] == 256


def test_the_figures_design_md_states(kernels):
    """`gfw_gyro_cost_kernel` 18 VGPR / 46 SGPR / no LDS, `gfw_gyro_pick_kernel` 12 VGPR / 32 SGPR / 3080 B LDS (256 x (f64 cost, index), the pick)"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for tag in ("gfw_gyro_cost_kernel", "gfw_gyro_pick_kernel"):
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % tag, text)
        assert m, "DESIGN.md does not state the figures of %s" % tag
        k = one(kernels, tag)
        got = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert got == tuple(int(v) for v in m.groups()), (tag, got, m.groups())
    assert one(kernels, "gfw_gyro_cost_kernel")[".group_segment_fixed_size"] == 0
    assert KR.waves_per_simd(one(kernels, "gfw_gyro_cost_kernel")[".vgpr_count"]) == 8              # a lane is a candidate: every wave a SIMD can hold


def test_every_kernel_that_existed_before_keeps_its_figures(kernels):
    """The fixture records ONE commit: the build before gfw_sync_gyro.hip was added.  It shows that adding the unit moved no earlier kernel; it is not a budget for
    those kernels (their own tests pin what matters about them).  A later change that moves an earlier kernel ON PURPOSE regenerates the fixture from its parent's
    build (tests/golden/kernel_resources_before_sync_gyro.py) or retires this test."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_sync_gyro.json")))["kernels"]
    assert len(before) > 300
    missing = sorted(n for n in before if n not in kernels)
    assert not missing, missing[:5]
    fig = lambda k: [k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]]
    moved = {n: (fig(kernels[n]), want) for n, want in before.items() if fig(kernels[n]) != want}
    assert not moved, moved
    assert not any("gfw_gyro_" in n for n in before)
