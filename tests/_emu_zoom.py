"""TEST INFRASTRUCTURE: the zoom search's kernel SOURCE (gyroflow_amd/csrc/gfw_zoom.hip and the headers it shares with the points kernel and the
matrix builder) interpreted on the host, the way tests/_emu.py runs gfw_points_kernel and gfw_matrices.hip: tests/emu/emu_zoom_driver.inc behind the
unedited source, the lanes of a frame's workgroup as cooperative fibers that rendezvous at __syncthreads.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import abi
import _emu

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_zoom.hip", n_asm=2, driver="emu_zoom_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_zoom.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, C.c_double, vp, vp, i32, vp, vp, vp]
        L.gfw_emu_zoom_table.argtypes = [vp, vp, i32, i32, i32, i32, C.c_float, vp]
        _lib = L
    return _lib


def zoom_fovs(params, model, digital, search, frames, rotations=None, tracks=None, offsets=None, duration_ms=1.0, debug=True):
    """gfw_zoom_fovs through the host-interpreted gfw_zoom_kernel -> (fov_minimal [n] f64, debug polygons [n][120][2] f64 or None).
    search: abi.ZoomSearch; frames: ctypes array of abi.ZoomFrame; tracks: (org, smoothed) as Backend.set_quaternion_tracks takes them, or None."""
    n = len(frames)
    com = _emu.common_for(_emu._Lenses(model, digital), params)
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data if a.size else None
    if tracks is not None:
        (ot, oq), (st, sq) = tracks
        targs = [arr(ot, np.int64), arr(oq, np.float64), len(ot), arr(st, np.int64), arr(sq, np.float64), len(st)]
    else:
        targs = [None, None, 0, None, None, 0]
    if offsets:
        targs += [arr(offsets[0], np.int64), arr(offsets[1], np.float64), len(offsets[0])]
    else:
        targs += [None, None, 0]
    fov = np.zeros(n, dtype=np.float64)
    dbg = np.zeros((n, 120, 2), dtype=np.float64) if debug else None
    rp = arr(np.asarray(rotations, dtype=np.float32).reshape(-1, 9), np.float32) if rotations is not None else None
    rc = lib().gfw_emu_zoom(C.cast(C.byref(params), C.c_void_p), C.cast(C.byref(com), C.c_void_p), *targs, float(duration_ms),
                            C.cast(C.byref(search), C.c_void_p), C.cast(frames, C.c_void_p), n, rp, fov.ctypes.data, dbg.ctypes.data if debug else None)
    assert rc == 0, "gfw_emu_zoom -> %d" % rc
    return fov, dbg


def zoom_table(outline, refined, width, height, org_output_size, margin=0.0):
    """The round logic and the fold of the kernel source over tabulated polygons (the point map replaced by a table): outline [120][2] f32, refined
    [4][63][2] f32 (what the k-th refinement maps to) -> fov f64."""
    o = np.ascontiguousarray(outline, dtype=np.float32).reshape(120, 2)
    r = np.ascontiguousarray(refined, dtype=np.float32).reshape(4, 63, 2)
    fov = C.c_double(0.0)
    rc = lib().gfw_emu_zoom_table(o.ctypes.data, r.ctypes.data, width, height, org_output_size[0], org_output_size[1], float(margin), C.byref(fov))
    assert rc == 0, "gfw_emu_zoom_table -> %d" % rc
    return fov.value
