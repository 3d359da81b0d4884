#!/usr/bin/env python3
"""Generate tests/golden/ref_coeffs.json: the reference's literal 32-phase tap table (`COEFFS` of src/core/stabilization/cpu_undistort.rs,
its first 448 entries: bilinear, bicubic, Lanczos4), the numbers tests/test_coeffs.py holds tools/gen_coeffs.py to bit for bit.

usage: python tests/golden/make_ref_coeffs.py <root of the reference's source tree>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
N = 448


def main(ref_root):
    rel = os.path.join("src", "core", "stabilization", "cpu_undistort.rs")
    src = open(os.path.join(ref_root, rel)).read()
    m = re.search(r"pub const COEFFS.*?= \[(.*?)\];", src, re.S)
    body = re.sub(r"//.*", "", m.group(1))
    vals = [float(t) for t in body.replace("\n", " ").split(",") if t.strip()][:N]
    assert len(vals) == N, len(vals)
    out = {"source": "COEFFS of %s (first %d entries: bilinear 32x2, bicubic 32x4, Lanczos4 32x8), as printed there" % (rel.replace(os.sep, "/"), N),
           "coeffs": vals}
    with open(os.path.join(HERE, "ref_coeffs.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
