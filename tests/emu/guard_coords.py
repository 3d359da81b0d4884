"""TEST INFRASTRUCTURE (run by tests/test_emu_coords.py, one process per placement): cases of tests/_coordcase.py through the host-interpreted gfw_stmap_kernel
with the coordinate map, the matrix table and the lens mesh placed flush against an inaccessible page — `end`: the buffer's last byte is the last accessible
one, `start`: its first byte the first.  A single byte read or written outside them kills this process with SIGSEGV; otherwise it prints OK per case (MISMATCH
where the map is not the oracle's).
usage: guard_coords.py end|start <case> [<case> ...]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _emu, _oracle as O, _coordcase as K
_emu.GUARD = sys.argv[1]
assert _emu.GUARD in ("end", "start")
for name in sys.argv[2:]:
    fr, kp, mesh, w, h = K.case(name)
    ref = O.stmap_undistort(kp, fr.model, fr.digital, fr.matrices, w, h, mesh=mesh, fill=K.SENTINEL)
    got = _emu.stmap_undistort(kp, fr.model, fr.digital, fr.matrices, w, h, mesh=mesh, fill=K.SENTINEL)
    print("OK" if np.array_equal(ref.view(np.uint32), got.view(np.uint32)) else "MISMATCH", flush=True)
