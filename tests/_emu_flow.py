"""TEST INFRASTRUCTURE: the optical flow's kernel SOURCE (gyroflow_amd/csrc/gfw_flow.hip) and the entry point's host code (gfw_flow_check, gfw_flow_plan,
gfw_flow_fill: gfw_flow_host.h) interpreted on the host, the way tests/_emu_pose.py runs gfw_pose.hip: tests/emu/emu_flow_driver.inc behind the unedited source,
the lanes of a workgroup as cooperative fibers that rendezvous at __syncthreads, at every __ballot and at every atomic.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import warp
import _emu

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_flow.hip", n_asm=0, driver="emu_flow_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_flow.argtypes = [i32, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


class Refused(ValueError):
    pass


def flow_pyrlk(frames, width, pairs, features=None, guard="end", iters=True, grid_outputs=True, reserved=0, mode=None, feat_first=None, n_frames=None):
    """gfw_flow_pyrlk through the host-interpreted kernels -> dict shaped as Backend.flow_pyrlk's; raises Refused with the reason where the entry point's own check
    refuses the arguments.  ``frames`` u8 [n][height][stride]; ``guard``: "end" / "start" / None — the frames and every pyramid level lie with their last / first
    byte against an inaccessible page."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, height, stride = frames.shape if frames.ndim == 3 else (0, 0, 0)
    n = n if n_frames is None else n_frames
    mode = (1 if features is None else 0) if mode is None else mode
    pf = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    ff, ft = (None, None) if features is None else warp.Backend._flow_features(features)
    if feat_first is not None:
        ff = np.ascontiguousarray(feat_first, dtype=np.int32)
    raw = max(0, warp.flow_raw_slots(width, height, pf, ff if mode == 0 else None)) if frames.size and pf.size and width >= 15 and (mode == 1 or ff is not None) else 0
    nodes = warp.flow_grid_nodes(width, height) if width >= 15 else 0
    o = {"next": np.full((raw, 2), -7.0, dtype=np.float32), "status": np.full(raw, 7, dtype=np.uint8), "iters": np.full((raw, 4), -7, dtype=np.int32),
         "pair_first": np.full(len(pf) + 1, -7, dtype=np.int32), "points_a": np.full((raw, 2), -7.0, dtype=np.float32), "points_b": np.full((raw, 2), -7.0, dtype=np.float32),
         "grid_points": np.full((max(n, 0), nodes, 2), -7.0, dtype=np.float32), "grid_counts": np.full(max(n, 0), -7, dtype=np.int32)}
    keep = frames
    if guard and frames.size:
        keep = _emu.guarded(frames, guard == "end")
    why = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib().gfw_emu_flow(width, height, stride, mode, reserved, keep.ctypes.data if frames.size else None, n, p(pf), len(pf), p(ff), p(ft),
                            p(o["next"]), p(o["status"]), p(o["iters"]) if iters else None, p(o["grid_points"]) if grid_outputs and mode == 1 else None,
                            p(o["grid_counts"]) if grid_outputs and mode == 1 else None, o["pair_first"].ctypes.data, p(o["points_a"]), p(o["points_b"]),
                            {"end": 1, "start": 2, None: 0}[guard], why, len(why))
    if rc == -1:
        raise Refused(why.value.decode())
    assert rc == 0, "gfw_emu_flow -> %d" % rc
    if len(pf):
        kept = int(o["pair_first"][-1])
        assert (o["points_a"][kept:] == -7.0).all() and (o["points_b"][kept:] == -7.0).all(), "the compaction wrote behind the kept points"
        o["points_a"], o["points_b"] = o["points_a"][:kept], o["points_b"][:kept]
    return o
