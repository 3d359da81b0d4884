"""TEST INFRASTRUCTURE: the corner detection's kernel SOURCE (gyroflow_amd/csrc/gfw_corners.hip) and the entry point's host code (gfw_corners_check,
gfw_corners_plan, gfw_corners_fill, gfw_corners_batch: gfw_corners_host.h) interpreted on the host, the way tests/_emu_flow.py runs gfw_flow.hip:
tests/emu/emu_corners_driver.inc behind the unedited source, the lanes of a workgroup as cooperative fibers that rendezvous at __syncthreads, at every __ballot and
at every atomic.  Not a product path."""
import ctypes as C

import numpy as np

import _emu

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_corners.hip", n_asm=0, driver="emu_corners_driver.inc", extra_flags=()))
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        L.gfw_emu_corners.argtypes = [i32, i32, i32, i32, f32, f32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


class Refused(ValueError):
    pass


def corners(frames, width, max_corners=200, quality=0.01, min_distance=10.0, scores=True, packed=True, max_workspace_mb=0, guard="end", reserved=0, n_frames=None,
            height=None, stride=None, null=()):
    """gfw_corners_shi_tomasi through the host-interpreted kernels -> dict shaped as Backend.corners_shi_tomasi's, plus info (batches, frames of a full batch,
    launches) and cand_counts; raises Refused with the reason where the entry point's own check refuses the arguments.  ``frames`` u8 [n][height][stride];
    ``guard``: "end" / "start" / None — the frames and the candidate lists lie with their last / first byte against an inaccessible page.  Every output is filled
    with a sentinel first (-7): what the call leaves untouched shows.  ``null``: names of arguments passed as NULL."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, s = frames.shape if frames.ndim == 3 else (0, 0, 0)
    n = n if n_frames is None else n_frames
    h, s = (h if height is None else height), (s if stride is None else stride)
    m = max_corners if 0 < max_corners <= 4096 else 1
    room = max(n, 0) * m
    o = {"corners": np.full((max(n, 0), m, 2), -7.0, dtype=np.float32), "scores": np.full((max(n, 0), m), -7.0, dtype=np.float32), "counts": np.full(max(n, 0), -7, dtype=np.int32),
         "feat_first": np.full(max(n, 0) + 1, -7, dtype=np.int32), "features": np.full((room, 2), -7.0, dtype=np.float32),
         "info": np.full(3, -7, dtype=np.int32), "cand_counts": np.full(max(n, 0), -7, dtype=np.int32)}
    keep = frames
    if guard and frames.size:
        keep = _emu.guarded(frames, guard == "end")
    why = C.create_string_buffer(512)
    p = lambda name, on=True: o[name].ctypes.data if on and name not in null else None
    rc = lib().gfw_emu_corners(width, h, s, max_corners, quality, min_distance, max_workspace_mb, reserved, keep.ctypes.data if frames.size and "frames" not in null else None, n,
                               p("corners"), p("scores", scores), p("counts"), p("feat_first", packed), p("features", packed),
                               {"end": 1, "start": 2, None: 0}[guard], o["info"].ctypes.data, o["cand_counts"].ctypes.data if n > 0 else None, why, len(why))
    if rc == -1:
        raise Refused(why.value.decode(), o)
    assert rc == 0, "gfw_emu_corners -> %d" % rc
    if packed and n > 0 and "feat_first" not in null:
        kept = int(o["feat_first"][-1])
        assert (o["features"][kept:] == -7.0).all(), "the pack wrote behind the kept corners"
        o["features"] = o["features"][:kept]
    return o
