"""What the tests/test_kernel_resources*.py files share: the kernels of the built libgfwarp.so as tools/kernel_resources.py reads them from its code objects (no GPU
needed), read once per run, and the checks every unit's file makes of its own kernels.  Each unit's own figures, counts and bounds stay in its file."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR          # noqa: E402

LIB = os.path.join(ROOT, "gyroflow_amd", "libgfwarp.so")
_kernels = None


def load():
    """{mangled name: metadata} of every kernel of the library"""
    global _kernels
    assert os.path.exists(LIB), "libgfwarp.so not built"
    if _kernels is None:
        _kernels = {k[".name"]: k for k in KR.report(LIB)}
    return _kernels


@pytest.fixture(scope="module")
def kernels():
    """the fixture of the per-unit files (imported by name): a missing library fails them; tests/test_kernel_resources.py has its own, which skips"""
    return load()


def one(kernels, tag):
    hits = [k for n, k in kernels.items() if tag in n]
    assert len(hits) == 1, (tag, len(hits))
    return hits[0]


def figures(k):
    return (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])


def design_md_figures(name):
    """the (V, S, L, X) of the line of DESIGN.md that names `name` with `V VGPR / S SGPR / L B LDS / X B scratch`"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        m = re.search(r"`%s`[^\n]*?(\d+) VGPR / (\d+) SGPR / (\d+) B LDS / (\d+) B scratch" % re.escape(name), f.read())
    assert m, "DESIGN.md does not state the figures of %s" % name
    return tuple(int(v) for v in m.groups())


def assert_design_md_figures(kernels, tags, names={}):
    """every kernel of `tags` is at the figures DESIGN.md states for it, there under names.get(tag, tag)"""
    for tag in tags:
        want, got = design_md_figures(names.get(tag, tag)), figures(one(kernels, tag))
        assert got == want, (tag, got, want)


def assert_no_scratch(kernels, names):
    """no scratch, no spills and no dynamic stack in any of the kernels `names`"""
    for n in names:
        assert kernels[n][".private_segment_fixed_size"] == 0, n
        assert kernels[n].get(".vgpr_spill_count", 0) == 0 and kernels[n].get(".sgpr_spill_count", 0) == 0, n
        assert not kernels[n].get(".uses_dynamic_stack", False), n
