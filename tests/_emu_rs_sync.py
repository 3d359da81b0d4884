"""TEST INFRASTRUCTURE: the rs-sync search's kernel SOURCE (gyroflow_amd/csrc/gfw_sync_rs.hip) and the entry points' host code (gfw_rs_check, gfw_rs_layout,
gfw_rs_fill, gfw_rs_constants, gfw_rs_round: gfw_sync_rs_host.h) interpreted on the host, the way tests/_emu_pose_essential.py runs gfw_pose_essential.hip:
tests/emu/emu_sync_rs_driver.inc behind the unedited source, the lanes of a workgroup as cooperative fibers that rendezvous at __syncthreads and at every shuffle of
the wave's butterfly.  Not a product path."""
import ctypes as C

import numpy as np

from gyroflow_amd import abi, warp
import _emu

# in front of the source: the cost stage's dynamic LDS as a static array of the largest size (3 x GFW_RS_PAIR_MAX doubles), and __shfl_xor of a double as a rendezvous of
# the wave's live lanes — a lane deposits its value, all arrive, it reads its partner's; the two buffers alternate, so one rendezvous a shuffle is enough: nobody
# deposits for shuffle k + 2 before everybody has read shuffle k
HEADER = """
#define GFW_RS_DYN_LDS(name) static double name[3 * 4096]
static double emu_shfl_buf[2][4][64];
static int emu_shfl_turn[4][64];
static inline double emu_shfl_xor(double v, int off, int site) {
    const int w = (int)threadIdx.y, l = (int)threadIdx.x, turn = emu_shfl_turn[w][l]++ & 1;
    emu_shfl_buf[turn][w][l] = v;
    emu_wave_sync(3000000 + site);
    return emu_shfl_buf[turn][w][l ^ off];
}
#define __shfl_xor(v, off) emu_shfl_xor(v, off, __LINE__)
"""
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_emu.build({}, HEADER, top="gfw_sync_rs.hip", n_asm=2, driver="emu_sync_rs_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_sync_rs.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32,
                                      C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


class Refused(ValueError):
    pass


def _call(params, model, digital, cfg, ranges, track_ts_us, track_wxyz, search, reals_tail, cand_first, cand, outs, guard):
    com = _emu.common_for(_emu._Lenses(model, digital), params)
    rf, ts, first, pa, pb = warp.Backend._sync_rs_ranges(ranges)
    tt, tq = np.ascontiguousarray(track_ts_us, dtype=np.int64).reshape(-1), np.ascontiguousarray(track_wxyz, dtype=np.float64).reshape(-1, 4)
    settings = np.array([cfg.rounds, cfg.refine, cfg.hypotheses, cfg.refits, cfg.jacobi_sweeps], dtype=np.int32)
    reals = np.array([cfg.frame_readout_time_ms, cfg.step_s, cfg.loss_scale] + list(reals_tail), dtype=np.float64)
    why = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib().gfw_emu_sync_rs(C.cast(C.byref(params), C.c_void_p), C.cast(C.byref(com), C.c_void_p), cfg.video_width, cfg.video_height, cfg.flow_width, cfg.flow_height,
                               settings.ctypes.data, reals.ctypes.data, search, rf.ctypes.data, len(ranges), p(ts), first.ctypes.data, p(pa), p(pb), len(ts),
                               p(tt), p(tq), len(tt), p(cand_first), p(cand), 0 if cand is None else len(cand), *[p(o) for o in outs], guard, why, len(why))
    if rc == -1:
        raise Refused(why.value.decode())
    assert rc == 0, "gfw_emu_sync_rs -> %d" % rc


def sync_rs_search(params, model, digital, cfg, ranges, track_ts_us, track_wxyz, initial_delay_s, radius_s, rounds=True, guard=1):
    """gfw_sync_rs_search through the host-interpreted kernels -> (rows (found, n_coarse, coarse_value, coarse_cost, value, cost), candidates, costs) shaped as the
    statement's (untouched outputs hold -7); raises Refused with the reason where the entry point's own check refuses the arguments"""
    n = len(ranges)
    total = warp.sync_rs_candidates(radius_s, cfg.step_s, cfg.rounds) if cfg.step_s > 0 and radius_s >= 0 and 1 <= cfg.rounds <= abi.SYNC_RS_ROUNDS_MAX else 1
    res, cand, cost = np.full((n, 5), -7.0), np.full((n, total), -7.0), np.full((n, total), -7.0)
    _call(params, model, digital, cfg, ranges, track_ts_us, track_wxyz, 1, [initial_delay_s, radius_s], None, None,
          [None, res, cand if rounds else None, cost if rounds else None], guard)
    ints = res[:, 0].copy().view(np.int32).reshape(-1, 2)
    return [(int(i[0]), int(i[1])) + tuple(r[1:]) for i, r in zip(ints, res)], cand, cost


def sync_rs_costs(params, model, digital, cfg, ranges, track_ts_us, track_wxyz, candidates, guard=1):
    """gfw_sync_rs_costs through the host-interpreted kernels -> one float64 cost array per range"""
    cands = [np.asarray(c, dtype=np.float64).reshape(-1) for c in candidates]
    cf = np.zeros(len(ranges) + 1, dtype=np.int32)
    if cands:
        cf[1:] = np.cumsum([len(c) for c in cands])
    cand = np.ascontiguousarray(np.concatenate(cands)) if cands else np.zeros(0)
    costs = np.full(max(len(cand), 1), -7.0)
    _call(params, model, digital, cfg, ranges, track_ts_us, track_wxyz, 0, [0.0, 0.0], cf, cand, [costs, None, None, None], guard)
    return [costs[cf[r]:cf[r + 1]].copy() for r in range(len(ranges))]
