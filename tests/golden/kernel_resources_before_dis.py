#!/usr/bin/env python3
"""Generator of kernel_resources_before_dis.json: registers / LDS / scratch of every kernel of a libgfwarp.so, as tools/kernel_resources.py reads them.

The committed file was taken from a build of the commit BEFORE the DIS dense optical flow (gfw_dis.hip) was added: tests/test_kernel_resources_dis.py holds
every kernel that existed then to these figures, so that the new translation unit is shown to have moved none of them.
usage: kernel_resources_before_dis.py <libgfwarp.so of that commit> [out.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tools"))
import kernel_resources as KR          # noqa: E402


def figures(lib):
    return {k[".name"]: [k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]] for k in KR.report(lib)}


if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "kernel_resources_before_dis.json")
    with open(out, "w") as f:
        json.dump({"columns": ["vgpr", "sgpr", "lds", "scratch"], "kernels": figures(sys.argv[1])}, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
