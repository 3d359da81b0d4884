"""TEST INFRASTRUCTURE: the essential-matrix pose estimation's kernel SOURCE (gyroflow_amd/csrc/gfw_pose_essential.hip) and the entry point's host code
(gfw_pose_ess_check, gfw_pose_ess_fill, gfw_pose_ess_constants: gfw_pose_essential_host.h) interpreted on the host, the way tests/_emu_pose.py runs gfw_pose.hip:
tests/emu/emu_pose_essential_driver.inc behind the unedited source, the lanes of a workgroup as cooperative fibers that rendezvous at __syncthreads and at every
__ballot.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import warp
import _emu

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_pose_essential.hip", n_asm=2, driver="emu_pose_essential_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_pose_essential.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_double, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


class Refused(ValueError):
    pass


def pose_essential(params, model, digital, cfg, pairs, octets, rounds=True):
    """gfw_pose_essential through the host-interpreted kernels -> (quats, rotations, essential, best, round_inliers, round_fits) shaped as Backend.pose_essential's
    (untouched outputs hold -7); raises Refused with the reason where the entry point's own check refuses the arguments"""
    com = _emu.common_for(_emu._Lenses(model, digital), params)
    first, pa, pb = warp.Backend._pose_pairs(pairs)
    n, iters = len(pairs), int(cfg.num_iters)
    oc = np.ascontiguousarray(octets, dtype=np.int32).reshape(-1)
    quats, rot, ess, best = np.full((n, 4), -7.0, dtype=np.float32), np.full((n, 3, 3), -7.0), np.full((n, 9), -7.0), np.full((n, 4), -7, dtype=np.int32)
    ri, rf = np.full((n, iters), -7, dtype=np.int32), np.full((n, iters, 9), -7.0)
    why = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib().gfw_emu_pose_essential(C.cast(C.byref(params), C.c_void_p), C.cast(C.byref(com), C.c_void_p), cfg.video_width, cfg.video_height, cfg.flow_width,
                                      cfg.flow_height, iters, cfg.inlier_threshold, cfg.min_front, first.ctypes.data, p(pa), p(pb), n, p(oc),
                                      p(quats), p(rot), p(ess), p(best), p(ri) if rounds else None, p(rf) if rounds else None, why, len(why))
    if rc == -1:
        raise Refused(why.value.decode())
    assert rc == 0, "gfw_emu_pose_essential -> %d" % rc
    return quats, rot, ess, best, ri, rf
