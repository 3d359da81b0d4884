"""Every kernel of the library against the record of one earlier build (tests/golden/kernel_resources.json: vgpr, sgpr, lds, scratch by mangled name), read from the
code objects inside libgfwarp.so (no GPU needed): a change that adds or refactors a translation unit has renamed and moved none of them."""
import json
import os

from _kres import ROOT, figures, kernels          # noqa: F401 (kernels: the fixture)


def test_every_recorded_kernel_is_present_at_its_recorded_figures(kernels):
    """The record is ONE build, every kernel of it (tests/golden/kernel_resources.py makes it).  It is not a budget for the kernels — their own files pin what matters
    about them — and it is never retaken to make this test pass: a change that moves or adds kernels ON PURPOSE retakes it from a build of its parent commit."""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")) as f:
        record = json.load(f)["kernels"]
    assert len(record) > 400
    missing = sorted(n for n in record if n not in kernels)
    assert not missing, missing[:5]
    moved = {n: (list(figures(kernels[n])), want) for n, want in record.items() if list(figures(kernels[n])) != want}
    assert not moved, moved
