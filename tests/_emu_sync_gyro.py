"""TEST INFRASTRUCTURE: the gyro-match search's kernel SOURCE (gyroflow_amd/csrc/gfw_sync_gyro.hip) and the entry points' host staging (gfw_gyro_stage,
gfw_sync_gyro_host.h) interpreted on the host, the way tests/_emu_sync.py runs gfw_sync.hip: tests/emu/emu_sync_gyro_driver.inc behind the unedited source, the lanes of
a workgroup as cooperative fibers that rendezvous at __syncthreads.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import abi, warp
import _emu
from _syncgyrostmt import lead_in

_lib = None
FINE = abi.SYNC_FINE_CANDIDATES


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_sync_gyro.hip", n_asm=0, driver="emu_sync_gyro_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_sync_gyro.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _run(ranges, candidates, search, initial_offset_ms, search_size_ms, lead=(0, 0, 0)):
    ef, e, eh, gf, g, gh = warp.Backend._sync_gyro_ranges(ranges)
    ef, e, eh = lead_in(ef, e, eh, lead[0], 1e9)
    gf, g, gh = lead_in(gf, g, gh, lead[1], -1e9)
    n = len(ranges)
    if search:
        n_coarse = warp.sync_gyro_coarse_count(search_size_ms)
        cf, cand, tot = None, None, n * n_coarse
    else:
        cands = [np.asarray(c, dtype=np.float64).reshape(-1) for c in candidates]
        cf = np.zeros(n + 1, dtype=np.int32)
        cf[1:] = np.cumsum([len(c) for c in cands])
        cand = np.ascontiguousarray(np.concatenate(cands)) if cands else np.zeros(0)
        cf, cand, _ = lead_in(cf, cand, None, lead[2], 12345.0)
        tot = len(cand)
    costs = np.full(max(tot, 1), -7.0)
    res = (abi.SyncResult * max(n, 1))()
    fine, fine_costs = np.full((max(n, 1), FINE), -7.0), np.full((max(n, 1), FINE), -7.0)
    kept = np.zeros(max(n, 1), dtype=np.int32)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib().gfw_emu_sync_gyro(ef.ctypes.data, p(e), p(eh), gf.ctypes.data, p(g), p(gh), n, p(cf) if cf is not None else None, p(cand), 1 if search else 0,
                                 float(initial_offset_ms), float(search_size_ms), costs.ctypes.data, C.cast(res, C.c_void_p), fine.ctypes.data, fine_costs.ctypes.data,
                                 kept.ctypes.data)
    assert rc == 0, "gfw_emu_sync_gyro -> %d" % rc
    return costs[:tot], cf, [res[i] for i in range(n)], fine[:n], fine_costs[:n], kept[:n]


def sync_gyro_costs(ranges, candidates, lead=(0, 0, 0), whole=False):
    """gfw_sync_gyro_costs through the host-interpreted kernel -> one float64 cost array per range.  ``lead``: how far into their arrays the estimated samples, the
    gyro samples and the candidates start (est_first[0], gyro_first[0], cand_first[0]); ``whole``: also the whole cost array, which started as -7.0"""
    costs, cf, _, _, _, _ = _run(ranges, candidates, False, 0.0, 0.0, lead)
    per = [costs[cf[r]:cf[r + 1]].copy() for r in range(len(ranges))]
    return (per, costs) if whole else per


def sync_gyro_search(ranges, initial_offset_ms, search_size_ms, lead=(0, 0, 0)):
    """gfw_sync_gyro_search through the host-interpreted kernels -> ([abi.SyncResult], coarse costs [n_ranges][n_coarse], fine candidates [n_ranges][200],
    fine costs [n_ranges][200], gyro entries each range kept)"""
    costs, _, res, fine, fine_costs, kept = _run(ranges, None, True, initial_offset_ms, search_size_ms, lead)
    return res, costs.reshape(len(ranges), warp.sync_gyro_coarse_count(search_size_ms)), fine, fine_costs, kept
