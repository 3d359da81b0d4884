"""TEST INFRASTRUCTURE: the sync search's kernel SOURCE (gyroflow_amd/csrc/gfw_sync.hip and the headers it shares with the points kernel, the matrix builder and
the zoom search) interpreted on the host, the way tests/_emu_zoom.py runs gfw_zoom.hip: tests/emu/emu_sync_driver.inc behind the unedited source, the lanes of a
workgroup as cooperative fibers that rendezvous at __syncthreads and at every __ballot.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import abi, warp
import _emu

_lib = None
FINE = abi.SYNC_FINE_CANDIDATES


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_sync.hip", n_asm=2, driver="emu_sync_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        f64 = C.c_double
        L.gfw_emu_sync.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, f64, vp, vp, vp, vp, vp, i32, vp, i32, i32, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp, vp]
        L.gfw_emu_sync_table.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp]
        L.gfw_emu_sync_point_split.argtypes = [vp, vp, vp, vp, i32, vp, vp]
        L.gfw_emu_sync_point_split.restype = None
        _lib = L
    return _lib


def _run(params, model, digital, search, pairs, candidates, mode, tracks, offsets, duration_ms, want_mapped, how=(0.0, 0.0, 0.0, 30.0)):
    """candidates: [n][2] (mode < 0), or the count of coarse candidates the search of `how` = (initial_offset_ms, search_size_ms, frame_readout_time_ms, scaled_fps) makes"""
    com = _emu.common_for(_emu._Lenses(model, digital), params)
    ts, first, pa, pb = warp.Backend._sync_pairs(pairs)
    total, n_pairs = int(first[-1]), len(pairs)
    cand = np.ascontiguousarray(candidates, dtype=np.float64).reshape(-1, 2) if mode < 0 else None
    n = cand.shape[0] if mode < 0 else int(candidates)
    (ot, oq), (st, sq) = tracks
    ot, st, oq, sq = (np.ascontiguousarray(ot, np.int64), np.ascontiguousarray(st, np.int64), np.ascontiguousarray(oq, np.float64), np.ascontiguousarray(sq, np.float64))
    use = bool(search.use_sync_offsets) and offsets is not None
    ft = np.ascontiguousarray(offsets[0], np.int64) if use else np.zeros(0, np.int64)
    fv = np.ascontiguousarray(offsets[1], np.float64) if use else np.zeros(0)
    rays = np.zeros((max(2 * total, 1), 4), dtype=np.float32)
    partial = np.zeros(max(n, FINE) * max(n_pairs, 1), dtype=np.uint64)
    fine, costs, fine_costs = np.zeros((FINE, 2)), np.full(max(n, 1), -7.0), np.full(FINE, -7.0)
    mapped = np.zeros((max(n, 1), max(total, 1), 2, 2), dtype=np.float32) if want_mapped else None
    res = abi.SyncResult()
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib().gfw_emu_sync(C.cast(C.byref(params), C.c_void_p), C.cast(C.byref(com), C.c_void_p), p(ot), p(oq), len(ot), p(st), p(sq), len(st), p(ft), p(fv), len(ft),
                            float(duration_ms), C.cast(C.byref(search), C.c_void_p), p(ts), first.ctypes.data, p(pa), p(pb), n_pairs, p(cand), n, mode, *[float(v) for v in how],
                            rays.ctypes.data, partial.ctypes.data, fine.ctypes.data, costs.ctypes.data, p(mapped), C.cast(C.byref(res), C.c_void_p) if mode >= 0 else None,
                            fine_costs.ctypes.data)
    assert rc == 0, "gfw_emu_sync -> %d" % rc
    return costs[:n], (mapped[:n, :total] if want_mapped else None), res, fine_costs, fine


def sync_visual_costs(params, model, digital, search, pairs, candidates, tracks, offsets=None, duration_ms=1.0, mapped=False):
    """gfw_sync_visual_costs through the host-interpreted kernels -> costs [n] f64 (, mapped [n][total][2][2] f32)"""
    costs, m, _, _, _ = _run(params, model, digital, search, pairs, candidates, -1, tracks, offsets, duration_ms, mapped)
    return (costs, m) if mapped else costs


def sync_visual_search(params, model, digital, search, pairs, mode, tracks, initial_offset_ms=0.0, search_size_ms=0.0, frame_readout_time_ms=0.0, scaled_fps=30.0,
                       offsets=None, duration_ms=1.0, fine=False):
    """gfw_sync_visual_search through the host-interpreted kernels -> (abi.SyncResult, coarse costs [n_coarse], fine costs [200]); the coarse candidates are made as
    the entry point makes them, by its own code.  fine: also the 200 fine candidates [200][2] the reduce stage wrote"""
    n = warp.sync_coarse_count(mode, search_size_ms, scaled_fps)
    costs, _, res, fine_costs, fine_cands = _run(params, model, digital, search, pairs, n, mode, tracks, offsets, duration_ms, False,
                                                 (initial_offset_ms, search_size_ms, frame_readout_time_ms, scaled_fps))
    return (res, costs, fine_costs, fine_cands) if fine else (res, costs, fine_costs)


def sync_table(mapped, pair_first, width, height, candidates=None, column=0):
    """The fold and the reduce stage of the kernel source over tabulated mapped points [n][total][2][2] f32 -> (costs [n] f64, abi.SyncResult, fine candidates [200][2])"""
    first = np.ascontiguousarray(pair_first, dtype=np.int32)
    n_pairs, total = len(first) - 1, int(first[-1])
    m = np.ascontiguousarray(mapped, dtype=np.float32).reshape(-1, max(total, 1) if total else 1, 2, 2) if np.size(mapped) else np.zeros((0, 1, 2, 2), np.float32)
    n = m.shape[0] if candidates is None else len(candidates)
    cand = np.ascontiguousarray(candidates if candidates is not None else [(float(i), 0.0) for i in range(n)], dtype=np.float64).reshape(-1, 2)
    partial = np.zeros(max(n, 1) * max(n_pairs, 1), dtype=np.uint64)
    fine, costs, res = np.zeros((FINE, 2)), np.full(max(n, 1), -7.0), abi.SyncResult()
    rc = lib().gfw_emu_sync_table(m.ctypes.data if m.size else None, first.ctypes.data, n_pairs, total, width, height, cand.ctypes.data if n else None, n, column,
                                  partial.ctypes.data, fine.ctypes.data, costs.ctypes.data, C.cast(C.byref(res), C.c_void_p))
    assert rc == 0, "gfw_emu_sync_table -> %d" % rc
    return costs[:n], res, fine


def point_split(params, model, digital, points, rotations):
    """gfw_point_map and its two halves composed over the same points -> (whole [n][2] f32, halves [n][2] f32)"""
    com = _emu.common_for(_emu._Lenses(model, digital), params)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    rot = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1, 9)
    assert len(rot) == len(pts)
    a, b = np.zeros_like(pts), np.zeros_like(pts)
    lib().gfw_emu_sync_point_split(C.cast(C.byref(params), C.c_void_p), C.cast(C.byref(com), C.c_void_p), pts.ctypes.data, rot.ctypes.data, len(pts), a.ctypes.data, b.ctypes.data)
    return a, b
