"""TEST INFRASTRUCTURE: gfw_flow_dis_refined's kernel SOURCE (gyroflow_amd/csrc/gfw_varref.hip, with gfw_dis.hip and the grid kernel of gfw_flow.hip) and the entry
point's host code (gfw_varref_check, gfw_varref_plan, gfw_varref_level: gfw_varref_host.h, on top of gfw_dis_host.h) interpreted on the host, the way
tests/_emu_dis.py runs gfw_dis.hip: tests/emu/emu_varref_driver.inc behind the unedited sources.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import warp
import _emu
import _varrefstmt as VS
from _emu_dis import Refused

_lib = None


def lib():
    global _lib
    if _lib is None:
        seen = set()                                      # gfw_image.h is included by all three units: once in the text
        header = _emu.kernel_source("gfw_flow.hip", 0, seen) + "\n" + _emu.kernel_source("gfw_dis.hip", 0, seen)
        L = C.CDLL(_emu.build({}, header, top="gfw_varref.hip", n_asm=0, driver="emu_varref_driver.inc", extra_flags=(), seen=seen))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_varref.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, C.c_char_p, C.c_size_t]
        L.gfw_emu_dis.argtypes = [i32, i32, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


def flow_dis_refined(frames, width, pairs, finest=2, cfg=VS.DEFAULT, guard="end", flow=True, variational_iters=0, reserved=0, ref_reserved=(0, 0), unrefined_call=False):
    """gfw_flow_dis_refined through the host-interpreted kernels -> dict shaped as Backend.flow_dis's, plus "launches"; raises Refused with the reason where the
    entry point's own check refuses.  ``frames`` u8 [n][height][stride]; ``cfg``: a _varrefstmt.Cfg; ``guard``: "end" / "start" / None — the frames, every array of
    both work spaces and every output lie with their last / first byte against an inaccessible page.  Every output starts as -7.  ``unrefined_call``: gfw_emu_dis
    of the same library instead (gfw_flow_dis's sequence)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, height, st = frames.shape
    pf = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    nodes = warp.flow_grid_nodes(width, height)
    shapes = {"grid_points": ((n, nodes, 2), np.float32), "grid_counts": ((n,), np.int32), "flow": ((len(pf), height >> finest, width >> finest, 2), np.float32),
              "pair_first": ((len(pf) + 1,), np.int32), "points_a": ((len(pf) * nodes, 2), np.float32), "points_b": ((len(pf) * nodes, 2), np.float32)}
    o = {}
    for name, (shape, dt) in shapes.items():
        a = np.full(shape, -7, dtype=dt)
        o[name] = _emu.guarded(a, guard == "end").view(dt).reshape(shape) if guard and a.size else a
    keep = _emu.guarded(frames, guard == "end") if guard else frames
    why = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    ints = np.array([cfg.fixed_point_iters, cfg.sor_iters, ref_reserved[0], ref_reserved[1]], dtype=np.int32)
    floats = np.array([cfg.alpha, cfg.delta, cfg.gamma, cfg.omega], dtype=np.float32)
    launches = np.zeros(1, dtype=np.int32)
    outs = (p(o["grid_points"]), p(o["grid_counts"]), p(o["flow"]) if flow else None, o["pair_first"].ctypes.data, p(o["points_a"]), p(o["points_b"]), {"end": 1, "start": 2, None: 0}[guard])
    if unrefined_call:
        rc = lib().gfw_emu_dis(width, height, st, finest, variational_iters, reserved, keep.ctypes.data, n, p(pf), len(pf), *outs, why, len(why))
    else:
        rc = lib().gfw_emu_varref(width, height, st, finest, variational_iters, reserved, ints.ctypes.data, floats.ctypes.data, keep.ctypes.data, n, p(pf), len(pf), *outs,
                                  launches.ctypes.data, why, len(why))
    o = {k: np.array(v) for k, v in o.items()}
    if rc == -1:
        e = Refused(why.value.decode())
        e.outputs = o
        raise e
    assert rc == 0, "gfw_emu_varref -> %d" % rc
    if len(pf):
        total = int(o["pair_first"][-1])
        assert (o["points_a"][total:] == -7.0).all() and (o["points_b"][total:] == -7.0).all(), "the node sampling wrote behind the returned points"
        o["points_a"], o["points_b"] = o["points_a"][:total], o["points_b"][:total]
    o["launches"] = int(launches[0])
    return o
