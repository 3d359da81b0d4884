"""Register / LDS / scratch figures of the sync-point choice's kernels (gyroflow_amd/csrc/gfw_sync_optim.hip) against what DESIGN.md section 3.2g states, read from
the code objects inside libgfwarp.so (no GPU needed): no scratch, no spills, and the documented numbers."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")
TAGS = ("gfw_optim_spectrum_kernel", "gfw_optim_max_kernel", "gfw_optim_rank_kernel", "gfw_optim_nms_kernel", "gfw_optim_pick_kernel", "gfw_optim_gather_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgfwarp.so not built"
    return {k[".name"]: k for k in KR.report(LIB)}


def one(kernels, tag):
    hits = [k for n, k in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, len(hits))
    return hits[0]


def test_the_new_kernels_are_six_and_use_no_scratch(kernels):
    new = sorted(n for n in kernels if "gfw_optim_" in n)
    assert len(new) == 6 and all(any(t in n for n in new) for t in TAGS), new
    assert not any("gfw_gyro_" in n for n in new)
    for n in new:
        assert kernels[n][".private_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert not kernels[n].get(".uses_dynamic_stack", False), n
        assert kernels[n][".max_flat_workgroup_size"] == 256


def test_the_figures_design_md_states(kernels):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for tag in TAGS:
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % tag, text)
        assert m, "DESIGN.md does not state the figures of %s" % tag
        k = one(kernels, tag)
        got = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert got == tuple(int(v) for v in m.groups()), (tag, got, m.groups())
    spectrum = one(kernels, "gfw_optim_spectrum_kernel")
    assert spectrum[".group_segment_fixed_size"] == 257 * 6 * 4 + 8 or spectrum[".group_segment_fixed_size"] == 257 * 6 * 4      # the round's bins (+ the dynamic part's alignment)
    assert KR.waves_per_simd(spectrum[".vgpr_count"]) == 8                                # registers do not limit the waves a SIMD holds: LDS does, at 18 N bytes a workgroup
    # the static part and the largest dynamic part fit the 160 KB of a gfx950 compute unit
    assert spectrum[".group_segment_fixed_size"] + 18 * 8192 <= 160 * 1024
