"""gfw_sync_rs_costs / gfw_sync_rs_search on the MI355X: the rs-sync offset search of all ranges in one device call, against the f64 statement
(tests/_rssyncstmt.py).  The arithmetic is one rounding per operator on both sides (+ - * / sqrt in f64) and every sum has one fixed order, so every comparison is
bit for bit: no tolerance.  The shapes are tests/_rssynccase.SPECS' "gpu" cases (the statement's results computed once and shared)."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as S, warp
import _pairbase as PB
import _rssynccase as RC
import _rssyncstmt as RS

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT
GPU_CASES = sorted(n for n in RC.SPECS if n.startswith("gpu-"))


def backend_for(cam):
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    return warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))


def search(be, c, **kw):
    return be.sync_rs_search(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1], c.initial_s, c.radius_s, **kw)


@pytest.mark.parametrize("name", GPU_CASES)
def test_the_device_equals_the_statement_to_the_bit(name):
    c = RC.case(name)
    be = backend_for(c.cam)
    res, cand, cost = search(be, c, rounds=True)
    assert warp.last_backend() == "sync_rs_search"
    RC.assert_search_equal((RC.rows_of(res), cand, cost), c.statement, name)
    assert [r[0] for r in c.statement[0]] == [1, 0, 1] and cand.shape[1] == RS.candidates_total(c.cfg, c.radius_s)
    RC.assert_search_equal((RC.rows_of(search(be, c)), c.statement[1], c.statement[2]), c.statement, name + " without round outputs")
    one = be.sync_rs_search(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges[2:], c.track[0], c.track[1], c.initial_s, c.radius_s, rounds=True)      # a range equals its own call
    RC.assert_search_equal((RC.rows_of(one[0]), one[1], one[2]), (c.statement[0][2:], c.statement[1][2:], c.statement[2][2:]), name + " range 2 alone")
    be.close()


def test_the_costs_of_the_searchs_own_candidates_equal_the_searchs_costs():
    c = RC.case("gpu-pinhole")
    be = backend_for(c.cam)
    want = c.statement
    got = be.sync_rs_costs(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1], [want[1][0], np.zeros(3), want[1][2][:5]])
    assert warp.last_backend() == "sync_rs_costs"
    assert [len(g) for g in got] == [want[1].shape[1], 3, 5]
    assert (RC.bits(got[0]) == RC.bits(want[2][0])).all() and (got[1] == 0.0).all() and (RC.bits(got[2]) == RC.bits(want[2][2][:5])).all()
    stmt = RS.costs_of(c.cam, c.cfg, c.track[0], c.track[1], c.ranges, [want[1][0][:4], [], [0.001, -0.5, 7.0]])      # candidates far outside the track too
    got = be.sync_rs_costs(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1], [want[1][0][:4], [], [0.001, -0.5, 7.0]])
    assert all((RC.bits(g) == RC.bits(w)).all() and len(g) == len(w) for g, w in zip(got, stmt))
    be.close()


@pytest.mark.parametrize("points", [abi.SYNC_RS_PAIR_POINTS_MAX, 2049, 2048])
def test_large_pairs_take_the_large_lds_path(points):
    """24 B a point of dynamic LDS: 2048 points are the last within the 48 KB a launch gets without asking, 4096 take 96 KB"""
    c = RC.case("gpu-pinhole")
    pin = c.cam
    big = [RC.plant_range(pin, [points, 3], 0.0073, 12.0, RC.unit((1.0, 0.4, 0.2), 0.5), 9, 0.3)]
    cand = [np.array([0.006, 0.0073])]
    be = backend_for(pin)
    got = be.sync_rs_costs(pin.kp, RC.cfg_of(pin, c.cfg), big, c.track[0], c.track[1], cand)
    want = RS.costs_of(pin, c.cfg, c.track[0], c.track[1], big, cand)
    assert (RC.bits(got[0]) == RC.bits(want[0])).all(), (got, want)
    be.close()


def device_outputs(n, total):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((n, 5), -7.0, dtype=torch.float64, device=dev), torch.full((n, total), -7.0, dtype=torch.float64, device=dev),
            torch.full((n, total), -7.0, dtype=torch.float64, device=dev))


def rows_of_tensor(t):
    """[n][5] f64 words of gfw_sync_result -> the statement's rows"""
    raw = t.cpu().numpy()
    ints = raw[:, 0].copy().view(np.int32).reshape(-1, 2)
    return [(int(i[0]), int(i[1])) + tuple(r[1:]) for i, r in zip(ints, raw)]


def test_host_and_device_outputs_agree():
    import torch
    assert C.sizeof(abi.SyncResult) == 40
    c = RC.case("gpu-pinhole")
    be = backend_for(c.cam)
    total = RS.candidates_total(c.cfg, c.radius_s)
    outs = device_outputs(len(c.ranges), total)
    torch.cuda.synchronize()
    assert search(be, c, out_ptrs=tuple(o.data_ptr() for o in outs)) is None
    RC.assert_search_equal((rows_of_tensor(outs[0]), outs[1].cpu().numpy(), outs[2].cpu().numpy()), c.statement, "device outputs")
    outs = device_outputs(len(c.ranges), total)
    torch.cuda.synchronize()
    assert search(be, c, out_ptrs=(outs[0].data_ptr(), None, None)) is None
    RC.assert_search_equal((rows_of_tensor(outs[0]), c.statement[1], c.statement[2]), c.statement, "device outputs without rounds")
    assert (outs[1].cpu().numpy() == -7.0).all() and (outs[2].cpu().numpy() == -7.0).all()
    n_cand = int(c.statement[1].size)
    costs = torch.full((n_cand,), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert be.sync_rs_costs(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1], list(c.statement[1]), out_ptr=costs.data_ptr()) is None
    be.synchronize()
    assert (RC.bits(costs.cpu().numpy().reshape(len(c.ranges), -1)) == RC.bits(c.statement[2])).all()
    be.close()


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots (two), other data each time, queued without waiting"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [RC.case("gpu-pinhole")] + [RC.Case("queued-%d" % k, RC.EC.pinhole_clip, "gpu", seed=5 + k, rounds=2) for k in range(1, abi.SYNC_RS_RING_SLOTS + 1)]
    be = backend_for(cases[0].cam)
    outs = [device_outputs(len(c.ranges), RS.candidates_total(c.cfg, c.radius_s)) for c in cases]
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for c, o in zip(cases, outs):
        search(be, c, out_ptrs=tuple(t.data_ptr() for t in o))
    be.synchronize()
    for c, o in zip(cases, outs):
        RC.assert_search_equal((rows_of_tensor(o[0]), o[1].cpu().numpy(), o[2].cpu().numpy()), c.statement, c.name + " queued")
    be.close()


def test_no_ranges_succeed_and_write_nothing():
    c = RC.case("gpu-pinhole")
    be = backend_for(c.cam)
    assert be.sync_rs_search(c.cam.kp, RC.cfg_of(c.cam, c.cfg), [], c.track[0], c.track[1], 0.0, 0.03) == []
    assert be.sync_rs_costs(c.cam.kp, RC.cfg_of(c.cam, c.cfg), [], c.track[0], c.track[1], []) == []
    be.close()


def test_every_rejection_names_its_range_or_pair_and_leaves_the_outputs_untouched():
    c = RC.case("gpu-pinhole")
    cam = c.cam
    be = backend_for(cam)
    rf, ts, first, pa, pb = warp.Backend._sync_rs_ranges(c.ranges)
    tt, tq = np.ascontiguousarray(c.track[0]), np.ascontiguousarray(c.track[1])
    n, total = len(c.ranges), RS.candidates_total(c.cfg, c.radius_s)
    res = np.full((n, 5), -7.0)
    outs = [res, np.full((n, total), -7.0), np.full((n, total), -7.0)]
    p = lambda a: None if a is None else a.ctypes.data

    def call(kp=None, cfg=None, rf_=rf, n_=n, ts_=ts, first_=first, pa_=pa, np_=len(ts), tt_=tt, tq_=tq, nt_=len(tt), initial=c.initial_s, radius=c.radius_s, outs_=None):
        o = outs_ or outs
        return be.lib.gfw_sync_rs_search(be.ctx, C.byref(kp or cam.kp), C.byref(cfg or RC.cfg_of(cam, c.cfg)), p(rf_), n_, p(ts_), p(first_), p(pa_), p(pb), np_,
                                         p(tt_), p(tq_), nt_, initial, radius, p(o[0]), p(o[1]), p(o[2]), 0)

    def refused(text, **kw):
        rc = call(**kw)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert all((o == -7.0).all() for o in outs)

    assert call() == 0                                                               # the arguments as they are succeed ..
    ints = res[:, 0].copy().view(np.int32).reshape(-1, 2)
    RC.assert_search_equal(([(int(i[0]), int(i[1])) + tuple(r[1:]) for i, r in zip(ints, res)], outs[1], outs[2]), c.statement, "raw call")
    for o in outs:
        o[...] = -7.0                                                                # .. and every variation below is refused
    refused("negative count", n_=-1)
    refused("negative count", np_=-1)
    refused("negative count", nt_=-1)
    refused("at most 65535", n_=abi.SYNC_RS_RANGES_MAX + 1)
    refused("at most 65535", np_=abi.SYNC_RS_PAIRS_MAX + 1)
    refused("without range_first", rf_=None)
    refused("range 0: range_first 1 is not 0", rf_=np.array([1, 7, 7, 10], dtype=np.int32))
    refused("range 1: range_first descends", rf_=np.array([0, 7, 6, 10], dtype=np.int32))
    refused("range 2: range_first ends at 9", rf_=np.array([0, 7, 7, 9], dtype=np.int32))
    refused("without pair_first", first_=None)
    refused("without pair_first / pair_ts_us", ts_=None)
    bad = first.copy(); bad[0] = -1
    refused("pair 0: pair_first -1 is negative", first_=bad)
    bad = first.copy(); bad[4] = bad[3] - 1
    refused("pair 3: pair_first descends", first_=bad)
    bad = first.copy(); bad[7:] += 4096
    refused("pair 6: 4296 points, at most 4096", first_=bad)
    refused("without points_a / points_b", pa_=None)
    refused("a track of 1 samples: at least 2", nt_=1)
    refused("a null track array", tq_=None)
    bad = tt.copy(); bad[100] = bad[99]
    refused("track sample 100: timestamp", tt_=bad)
    bad = tt.copy(); bad[7] = bad[5]
    refused("track sample 7: timestamp", tt_=bad)
    refused("a null result array", outs_=[None, outs[1], outs[2]])
    for step in (0.0, -0.003, float("nan"), float("inf")):
        cfg = RC.cfg_of(cam, c.cfg); cfg.step_s = step
        refused("step", cfg=cfg)
    refused("radius", radius=-0.001)
    refused("radius", radius=float("nan"))
    refused("initial delay", initial=float("inf"))
    refused("candidates", radius=1e9)
    for rounds in (0, abi.SYNC_RS_ROUNDS_MAX + 1):
        cfg = RC.cfg_of(cam, c.cfg); cfg.rounds = rounds
        refused("rounds, 1 .. 8", cfg=cfg)
    for field, value in (("hypotheses", 65), ("refits", -1), ("jacobi_sweeps", 0), ("loss_scale", 0.0)):
        cfg = RC.cfg_of(cam, c.cfg); setattr(cfg, field, value)
        refused("bad rs-sync configuration", cfg=cfg)
    for flag in (abi.FLAG_HAS_IBIS_DATA, abi.FLAG_HAS_MESH_DATA, abi.FLAG_HAS_FPD_DATA):
        kp = cam.kp.copy(); kp.flags |= flag
        refused("does not cover", kp=kp)
    kp = cam.kp.copy(); kp.f[0] = kp.f[0] + 1.0
    refused("not the f32 cast of camera_matrix", kp=kp)
    cfg = RC.cfg_of(cam, c.cfg); cfg.reserved[2] = 1
    refused("reserved", cfg=cfg)
    cfg = RC.cfg_of(cam, c.cfg); cfg.flow_height = 0
    refused("bad rs-sync configuration", cfg=cfg)
    # gfw_sync_rs_costs' own: the candidates
    costs = np.full(8, -7.0)

    def costs_refused(text, cf, cand, n_cand):
        rc = be.lib.gfw_sync_rs_costs(be.ctx, C.byref(cam.kp), C.byref(RC.cfg_of(cam, c.cfg)), p(rf), n, p(ts), p(first), p(pa), p(pb), len(ts), p(tt), p(tq), len(tt),
                                      p(cf), p(cand), n_cand, p(costs), 0)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg and (costs == -7.0).all(), (rc, text, msg)

    cand = np.zeros(8)
    costs_refused("without cand_first", None, cand, 8)
    costs_refused("range 0: cand_first 2 is not 0", np.array([2, 4, 6, 8], dtype=np.int32), cand, 8)
    costs_refused("range 1: cand_first descends", np.array([0, 4, 3, 8], dtype=np.int32), cand, 8)
    costs_refused("range 2: cand_first ends at 7", np.array([0, 4, 4, 7], dtype=np.int32), cand, 8)
    costs_refused("without their array", np.array([0, 4, 4, 8], dtype=np.int32), None, 8)
    be.close()


class Params:
    pass


def compute_params(cam, readout_ms, fps=RC.FPS):
    cp = Params()
    cp.lens, cp.width, cp.height, cp.output_width, cp.output_height = cam.clip.lens, cam.video[0], cam.video[1], cam.video[0], cam.video[1]
    cp.digital_lens_params, cp.light_refraction_coefficient, cp.scaled_fps, cp.frame_readout_time = [], 1.0, fps, readout_ms
    return cp


def matched_of(pairs):
    return {ta: (tb, a, b) for ta, tb, a, b in pairs}


def test_the_python_mirror_runs_end_to_end_from_the_fast_initial_offset_to_accepted_offsets():
    """synchronization.find_offsets_rssync: calc_initial_fast through initial_offset_fast (the gyro-match search of the planted rates: 3000 ms behind it, 2001
    candidates), collect_points' range cut, ranges under 2 pairs skipped, the readout rules, the sign and unit conventions, the 90 % rule and the middle
    timestamp — equal to the statement run from the same initial offset; the delay outside the search is refused; find_offsets dispatches method 2 here;
    guess_orientation picks the track that is the camera's"""
    c = RC.clip("d+7.3")
    cam, pairs = c.cam, c.ranges[0]
    be = backend_for(cam)
    cp = compute_params(cam, c.readout_ms)
    matched = matched_of(pairs)
    ranges = [(pairs[0][0], pairs[-1][0] + 1), (pairs[0][0], pairs[0][0] + 1), (5, 5)]       # all pairs; one pair (skipped); empty (skipped)
    # the planted angular rates (degrees a second) as the estimator's and as the gyro's, the gyro's clock ahead by the delay
    rate = lambda t: np.degrees((RC.rotvec(t + 0.0005) - RC.rotvec(t - 0.0005)) / 0.001)
    est = {int(ta + 16667): ((ta + 16667) / 1000.0, tuple(rate((ta + 16667) / 1e6 + c.delay_ms / 1000.0))) for ta, _, _, _ in pairs}
    imu = [(t * 1.0, tuple(rate(t / 1000.0))) for t in range(0, 4001)]
    sp = SY.SyncParams(initial_offset=0.0, search_size=100.0)
    initial, size = SY.initial_offset_fast(est, imu, 4000.0, RC.FPS, ranges[:1], sp, be)
    assert size == 3000.0, (initial, size)                                            # the gyro match found something: the search starts from its median
    got = SY.find_offsets_rssync(cp, ranges, matched, sp, be, c.track, calc_initial_fast=True, estimated_gyro=est, raw_imu=imu, duration_ms=4000.0, flow_size=cam.flow)
    assert warp.last_backend() == "sync_rs_search"
    want = RS.search(cam, c.cfg, c.track[0], c.track[1], [pairs], -initial / 1000.0, size / 1000.0)[0][0]
    assert want[1] == 2001 and len(got) == 1
    ts, offset, cost = got[0]
    assert ts == float(pairs[0][0] + pairs[-1][1]) / 2.0 / 1000.0
    assert offset == -(want[4] * 1000.0) - (c.readout_ms / 1000.0 * 1000.0 / 2.0) and cost == want[5]
    assert abs(offset - (-c.delay_ms - c.readout_ms / 2.0)) < 1.0, offset              # within a gyro sample period of the truth
    again = SY.find_offsets(2, cp, ranges, sp, be, matched_points=matched, track=c.track, calc_initial_fast=True, estimated_gyro=est, raw_imu=imu, duration_ms=4000.0, flow_size=cam.flow)
    assert again == got and SY.find_offsets(9, cp, ranges, sp, be) == []
    # the search's own radius, no fast start: accepted inside, refused outside
    sp = SY.SyncParams(initial_offset=0.0, search_size=c.radius_ms)
    inside = SY.find_offsets_rssync(cp, ranges[:1], matched, sp, be, c.track, flow_size=cam.flow)
    assert len(inside) == 1 and inside[0][1] == -(c.searched()[0][0][4] * 1000.0) - (c.readout_ms / 1000.0 * 1000.0 / 2.0)
    out = RC.clip("d-outside")
    assert SY.find_offsets_rssync(cp, ranges[:1], matched_of(out.ranges[0]), sp, be, out.track, flow_size=cam.flow) == []
    assert abs(out.searched()[0][0][4] * 1000.0) >= 0.9 * c.radius_ms                   # .. by the 90 % rule, not for want of a result
    # a readout of 0 becomes half a frame; a global shutter 0.01 ms
    assert SY.rs_readout_time_ms(compute_params(cam, 0.0)) == 1000.0 / RC.FPS / 2.0
    gs = compute_params(cam, 12.0); gs.lens = dict(cam.clip.lens, global_shutter=True)
    assert SY.rs_readout_time_ms(gs) == 0.01
    # the orientation guess: the camera's track against the same track mirrored in x, and the later of two equal tracks
    flipped = (c.track[0], c.track[1] * np.array([1.0, -1.0, 1.0, 1.0]))
    name, total = SY.guess_orientation({"XYZ": c.track, "xYZ": flipped}, cp, ranges[:1], matched, sp, be, flow_size=cam.flow)
    assert name == "XYZ" and total == c.searched()[0][0][3]
    assert SY.guess_orientation({"a": c.track, "b": c.track}, cp, ranges[:1], matched, sp, be, flow_size=cam.flow)[0] == "b"
    assert SY.guess_orientation({}, cp, ranges[:1], matched, sp, be, flow_size=cam.flow) is None
    be.close()


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged from 0 and the points from the third on (tests/_pairbase.py)"""
    c = PB.rs_sync()
    be = backend_for(c.cam)
    args = (c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1])
    costs = PB.assert_base_does_not_matter(lambda: be.sync_rs_costs(*args, c.candidates), "sync_rs_costs")
    assert len(costs[0]) == 3 and len(set(costs[0].tolist())) == 3 and all(v > 0.0 for v in costs[0])

    def searched():
        res, cand, cost = be.sync_rs_search(*args, c.initial_s, c.radius_s, rounds=True)
        return np.array(RC.rows_of(res)), cand, cost
    rows, cand, cost = PB.assert_base_does_not_matter(searched, "sync_rs_search")
    be.close()
    assert cand.shape == (1, 3) and rows[0][1] == 3 and len(set(cost[0].tolist())) == 3
