"""TEST INFRASTRUCTURE: the sync-point choice's kernel SOURCE (gyroflow_amd/csrc/gfw_sync_optim.hip) and the entry points' host arithmetic and staging
(gfw_optim_shape, gfw_optim_fill: gfw_sync_optim_host.h) interpreted on the host, the way tests/_emu_sync_gyro.py runs gfw_sync_gyro.hip:
tests/emu/emu_sync_optim_driver.inc behind the unedited source, the lanes of a workgroup as cooperative fibers that rendezvous at __syncthreads.  The one thing the
host build is told is where the spectrum stage's dynamic LDS lies: a static array of the largest size.  Not a product path."""
import ctypes as C

import numpy as np

import _emu

_lib = None
LDS = "#define GFW_OPTIM_DYN_LDS(name) static float4 name[8192 + 1024]      /* 16 N + 4 (N / 2) bytes at N = 8192 */\n"


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, LDS, top="gfw_sync_optim.hip", n_asm=0, driver="emu_sync_optim_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_sync_optim.argtypes = [vp, C.c_longlong, C.c_double, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def run(gyro, sample_rate, target=0, trims=(), points=True):
    """gfw_sync_optim_points (or, points False, gfw_sync_optim_rank) through the host-interpreted kernels -> dict of lf, mf, hf, rank, masked, rank_nms (f32
    [n_windows]), points (f64), shape (fft_size, n_windows, nms_radius, segment_size, bin[4]); every array started as -7 and holds what the kernels wrote"""
    g = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1))
    s = g.shape[1]
    tr = np.ascontiguousarray(np.asarray(trims, dtype=np.float64).reshape(-1, 2))
    shape = np.zeros(8, dtype=np.int32)
    cap = s // 16 + 2
    arr = {k: np.full(cap, -7.0, dtype=np.float32) for k in ("lf", "mf", "hf", "rank", "masked", "rank_nms")}
    pts = np.full(max(target, 1), -7.0)
    n_points = np.full(1, -7, dtype=np.int32)
    rc = lib().gfw_emu_sync_optim(g.ctypes.data if s else None, s, float(sample_rate), 1 if points else 0, int(target), tr.ctypes.data if len(tr) else None, len(tr),
                                  *[arr[k].ctypes.data for k in ("lf", "mf", "hf", "rank", "masked", "rank_nms")], pts.ctypes.data, n_points.ctypes.data, shape.ctypes.data)
    assert rc == 0, "gfw_emu_sync_optim -> %d" % rc
    w = int(shape[1])
    out = {k: v[:w].copy() for k, v in arr.items()}
    assert all(np.all(v[w:] == -7.0) for v in arr.values())                     # nothing behind the windows is written
    if points:
        assert 0 <= n_points[0] <= target, n_points
        out["points"] = pts[:n_points[0]].copy()
        assert np.all(pts[n_points[0]:] == -7.0)
    out["shape"] = shape
    return out
