"""TEST INFRASTRUCTURE: the DIS dense flow's kernel SOURCE (gyroflow_amd/csrc/gfw_dis.hip, and gfw_flow.hip for the grid kernel it shares) and the entry point's host
code (gfw_dis_check, gfw_dis_plan, gfw_dis_fill: gfw_dis_host.h) interpreted on the host, the way tests/_emu_flow.py runs gfw_flow.hip: tests/emu/emu_dis_driver.inc
behind the unedited sources, the lanes of a workgroup as cooperative fibers that rendezvous at __syncthreads, at every __ballot and at every atomic.  Not a product
path."""
import ctypes as C

import numpy as np

from gyroflow_amd import warp
import _emu

_lib = None


def lib():
    global _lib
    if _lib is None:
        seen = set()                                      # gfw_image.h is included by both units: once in the text
        L = C.CDLL(_emu.build({}, _emu.kernel_source("gfw_flow.hip", 0, seen), top="gfw_dis.hip", n_asm=0, driver="emu_dis_driver.inc", extra_flags=(), seen=seen))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_dis.argtypes = [i32, i32, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


class Refused(ValueError):
    pass


def flow_dis(frames, width, pairs, finest=2, guard="end", grid_outputs=True, flow=True, variational_iters=0, reserved=0, n_frames=None, stride=None):
    """gfw_flow_dis through the host-interpreted kernels -> dict shaped as Backend.flow_dis's; raises Refused with the reason where the entry point's own check
    refuses the arguments.  ``frames`` u8 [n][height][stride]; ``guard``: "end" / "start" / None — the frames, every array of the work space and every output lie
    with their last / first byte against an inaccessible page.  Every output starts as -7: what the call leaves untouched still is."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, height, st = frames.shape if frames.ndim == 3 else (0, 0, 0)
    n = n if n_frames is None else n_frames
    st = st if stride is None else stride
    pf = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    sane = width >= 16 and height >= 16 and finest in (1, 2)
    nodes = warp.flow_grid_nodes(width, height) if sane else 0
    fw, fh = (width >> finest, height >> finest) if sane else (0, 0)
    shapes = {"grid_points": ((max(n, 0), nodes, 2), np.float32), "grid_counts": ((max(n, 0),), np.int32), "flow": ((min(len(pf), 64), fh, fw, 2), np.float32),
              "pair_first": ((len(pf) + 1,), np.int32), "points_a": ((min(len(pf), 64) * nodes, 2), np.float32), "points_b": ((min(len(pf), 64) * nodes, 2), np.float32)}
    o = {}
    for name, (shape, dt) in shapes.items():
        a = np.full(shape, -7, dtype=dt)
        o[name] = _emu.guarded(a, guard == "end").view(dt).reshape(shape) if guard and a.size else a
    keep = _emu.guarded(frames, guard == "end") if guard and frames.size else frames
    why = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib().gfw_emu_dis(width, height, st, finest, variational_iters, reserved, keep.ctypes.data if frames.size else None, n, p(pf), len(pf),
                           p(o["grid_points"]) if grid_outputs else None, p(o["grid_counts"]) if grid_outputs else None, p(o["flow"]) if flow else None,
                           o["pair_first"].ctypes.data, p(o["points_a"]), p(o["points_b"]), {"end": 1, "start": 2, None: 0}[guard], why, len(why))
    o = {k: np.array(v) for k, v in o.items()}
    if rc == -1:
        e = Refused(why.value.decode())
        e.outputs = o
        raise e
    assert rc == 0, "gfw_emu_dis -> %d" % rc
    if len(pf):
        total = int(o["pair_first"][-1])
        assert (o["points_a"][total:] == -7.0).all() and (o["points_b"][total:] == -7.0).all(), "the node sampling wrote behind the returned points"
        o["points_a"], o["points_b"] = o["points_a"][:total], o["points_b"][:total]
    return o
