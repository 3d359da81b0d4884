"""gfw_sync_optim_rank / gfw_sync_optim_points on the MI355X: where in a clip to sync, one device call, against the f32 statement (tests/_syncoptimstmt.py).  A bin
is a sequential f32 fold whatever the launch shape, and everything behind it is the reference's own f32 arithmetic, so every comparison is bit for bit: no
tolerance.  The shapes are the interpreter tier's (tests/test_emu_sync_optim.py); one clip has a real size (1 kHz, 20 s: 1188 windows)."""
import ctypes as C
import math

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as SF, warp
import _syncoptimstmt as S
from test_emu_sync_optim import noise, tone

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT
ALL = ((0.0, 1e9),)


@pytest.fixture()
def be():
    fr = SF.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    b = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    yield b
    b.close()


def check(be, gyro, rate, target, trims=ALL):
    pts, rank, ratio, nms = be.sync_optim_points(gyro, rate, target, trims, details=True)
    assert warp.last_backend() == "sync_optim_points"
    s = S.run_f32(gyro, rate, target, trims)
    assert ratio == s["ratio"] and S.same_bits(rank, s["rank"]) and S.same_bits(nms, s["rank_nms"]), (rate, target)
    assert S.same_bits(pts, s["points"]), (pts, s["points"])
    lf, mf, hf, rank2 = be.sync_optim_rank(gyro, rate)
    assert warp.last_backend() == "sync_optim_rank"
    assert S.same_bits(lf, s["lf"]) and S.same_bits(mf, s["mf"]) and S.same_bits(hf, s["hf"]) and S.same_bits(rank2, rank)
    return pts, rank, nms


def small_cases():
    """(gyro, rate, target, trims): the interpreter tier's shapes"""
    t = np.arange(32 + 16 * 5) / 32.0
    loud = tone(400, 100.0, 40.0, 4000.0) + tone(400, 100.0, 0.7, 9000.0) + tone(400, 100.0, 9.0, 60.0)
    two = tone(160 + 16 * 59, 160.0, 8.0, 50.0, seed=10, noise_scale=2.0)
    cases = [(noise(S.fft_size(r) + 16 * (w - 1) + 7, int(r)), r, 2, ALL) for r, w in ((16.0, 3), (97.3, 5), (200.0, 4), (520.0, 8))]
    cases += [(noise(32 + extra, 1), 32.0, 3, ALL) for extra in (-1, 0, 15, 16)]
    cases += [(tone(16 + 16 * 256, 16.0, 3.0, 40.0, seed=2, noise_scale=8.0), 16.0, target, ALL) for target in (1, 2, 300)]
    cases += [(noise(8192, 5), 8192.0, 1, ALL), (noise(50 + 40, 6), 50.0, 1, ALL), (noise(4000, 7), 4000.0, 1, ALL),
              (noise(50 * 5, 8, scale=0.05), 50.0, 2, ALL), (np.zeros((3, 200)), 50.0, 3, ALL), (loud, 100.0, 2, ALL),
              (tone(160 + 16 * 118, 160.0, 8.0, 50.0, seed=9, noise_scale=2.0), 160.0, 3, ALL), (tone(160 + 16 * 120, 160.0, 8.0, 50.0, seed=9, noise_scale=2.0), 160.0, 3, ALL),
              (two, 160.0, 2, ()), (two, 160.0, 2, ((100.0, 200.0),)), (two, 160.0, 2, ((1.0, 1.5), (5.5, 5.7))),
              (tone(32 + 16 * 9, 32.0, 4.0, 50.0), 32.0, 3, ALL), (tone(32 + 16 * 9, 32.0, 4.0, 50.0), 32.0, 14, ALL),
              (tone(len(t), 32.0, 5.0, 90.0) * np.exp(-t / 2.0), 32.0, 2, ALL)]
    return cases


def test_the_interpreter_tiers_shapes_equal_the_statement(be):
    seen_points = 0
    for gyro, rate, target, trims in small_cases():
        pts, rank, nms = check(be, gyro, rate, target, trims)
        seen_points += len(pts)
    assert seen_points > 20


def test_a_one_khz_clip_of_twenty_seconds(be):
    g, centres = S.planted_clip(1000.0, 20.0)
    pts, rank, nms = check(be, g, 1000.0, 3, ((0.0, 20.0),))
    assert len(rank) == 1188 and len(pts) >= 2
    for c in (7.0, 19.0 - 12.0):
        pass
    assert min(abs(pts - 7000.0)) <= 2.0 * 16.0                                          # the burst at 7 s (19 s lies in the last two seconds' mask)


def device_outputs(target, n_w):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((max(target, 1),), -1.0, dtype=torch.float64, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev),
            torch.full((max(n_w, 1),), -1.0, dtype=torch.float32, device=dev), torch.full((max(n_w, 1),), -1.0, dtype=torch.float32, device=dev))


def test_host_and_device_outputs_agree_and_every_optional_output_may_be_null(be):
    import torch
    g, _ = S.planted_clip(200.0, 60.0)
    trims = ((0.0, 60.0),)
    pts, rank, ratio, nms = be.sync_optim_points(g, 200.0, 4, trims, details=True)
    n_w = len(rank)
    d_pts, d_n, d_rank, d_nms = device_outputs(4, n_w)
    torch.cuda.synchronize()
    assert be.sync_optim_points(g, 200.0, 4, trims, out_ptrs=(d_pts.data_ptr(), d_n.data_ptr(), d_rank.data_ptr(), d_nms.data_ptr())) == ratio
    be.synchronize()
    n = int(d_n.cpu()[0])
    assert n == len(pts) and S.same_bits(d_pts.cpu().numpy()[:n], pts) and np.all(d_pts.cpu().numpy()[n:] == -1.0)
    assert S.same_bits(d_rank.cpu().numpy()[:n_w], rank) and S.same_bits(d_nms.cpu().numpy()[:n_w], nms)
    # every optional output NULL: device and host
    d_pts2, d_n2, _, _ = device_outputs(4, n_w)
    torch.cuda.synchronize()
    gg = np.ascontiguousarray(g)
    tr = np.array(trims, dtype=np.float64)
    assert be.lib.gfw_sync_optim_points(be.ctx, gg.ctypes.data, gg.shape[1], 200.0, 4, tr.ctypes.data, 1, d_pts2.data_ptr(), d_n2.data_ptr(), None, None, None, 1) == 0
    be.synchronize()
    assert int(d_n2.cpu()[0]) == n and S.same_bits(d_pts2.cpu().numpy()[:n], pts)
    h_pts, h_n = np.full(4, -1.0), C.c_int32(-1)
    assert be.lib.gfw_sync_optim_points(be.ctx, gg.ctypes.data, gg.shape[1], 200.0, 4, tr.ctypes.data, 1, h_pts.ctypes.data, C.addressof(h_n), None, None, None, 0) == 0
    assert h_n.value == n and S.same_bits(h_pts[:n], pts)
    n_w_out = C.c_int32(-1)
    assert be.lib.gfw_sync_optim_rank(be.ctx, gg.ctypes.data, gg.shape[1], 200.0, None, None, None, None, C.addressof(n_w_out), 0) == 0 and n_w_out.value == n_w
    assert be.lib.gfw_sync_optim_rank(be.ctx, gg.ctypes.data, gg.shape[1], 200.0, None, None, None, None, None, 0) == 0
    d_rank3 = torch.full((n_w,), -1.0, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert be.sync_optim_rank(g, 200.0, out_ptrs=(None, None, None, d_rank3.data_ptr())) == n_w
    be.synchronize()
    assert S.same_bits(d_rank3.cpu().numpy(), rank)                                      # gfw_sync_optim_rank's rank is gfw_sync_optim_points's


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots(be):
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots, other data each time, queued without waiting; each result equals its lone
    synchronous call"""
    import torch
    dev = torch.device("cuda", 0)
    calls = abi.SYNC_OPTIM_RING_SLOTS + 1
    rates = [100.0, 200.0, 160.0, 97.3][:calls]
    data = [S.planted_clip(r, 30.0 + 5.0 * k, seed=20 + k)[0] for k, r in enumerate(rates)]
    alone = [be.sync_optim_points(data[k], rates[k], 3 + k, ALL, details=True) for k in range(calls)]
    outs = [device_outputs(3 + k, len(alone[k][1])) for k in range(calls)]
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for k in range(calls):
        be.sync_optim_points(data[k], rates[k], 3 + k, ALL, out_ptrs=tuple(o.data_ptr() for o in outs[k]))
    be.synchronize()
    for k in range(calls):
        pts, rank, ratio, nms = alone[k]
        d_pts, d_n, d_rank, d_nms = outs[k]
        n = int(d_n.cpu()[0])
        assert n == len(pts) and n > 0 and S.same_bits(d_pts.cpu().numpy()[:n], pts), k
        assert S.same_bits(d_rank.cpu().numpy(), rank) and S.same_bits(d_nms.cpu().numpy(), nms), k
    assert len({a[0].tobytes() for a in alone}) == calls                               # the calls did differ


def test_empty_cases_succeed_with_nothing(be):
    pts, rank, ratio = be.sync_optim_points(noise(99, 1), 100.0, 5, ALL)                 # fewer samples than a window
    assert len(pts) == 0 and len(rank) == 0 and ratio == 0.16
    pts, rank, ratio = be.sync_optim_points(np.zeros((3, 0)), 100.0, 5, ALL)
    assert len(pts) == 0 and len(rank) == 0
    assert all(len(a) == 0 for a in be.sync_optim_rank(noise(99, 1), 100.0))
    g = tone(160 + 16 * 59, 160.0, 8.0, 50.0, seed=10, noise_scale=2.0)
    assert len(be.sync_optim_points(g, 160.0, 2, ())[0]) == 0                            # `any` over nothing


def test_every_rejected_argument_names_its_reason_and_leaves_the_outputs_untouched(be):
    g = np.ascontiguousarray(noise(400, 3))
    tr = np.array([[0.0, 100.0]])
    pts, n_pts, rank, nms, ratio = np.full(8, -3.0), C.c_int32(-3), np.full(64, -3.0, dtype=np.float32), np.full(64, -3.0, dtype=np.float32), C.c_double(-3.0)
    lf, n_w = np.full(64, -3.0, dtype=np.float32), C.c_int32(-3)

    def points(ctx=be.ctx, gyro=g.ctypes.data, s=400, rate=100.0, target=4, trim=tr.ctypes.data, n_trim=1, p=pts.ctypes.data, n=C.addressof(n_pts)):
        return be.lib.gfw_sync_optim_points(ctx, gyro, s, rate, target, trim, n_trim, p, n, rank.ctypes.data, nms.ctypes.data, C.addressof(ratio), 0)

    def rejected(what, rc, *names):
        assert rc == INV, (what, rc)
        msg = be.lib.gfw_last_error().decode()
        for name in names:
            assert name in msg, (what, msg)
        assert np.all(pts == -3.0) and n_pts.value == -3 and np.all(rank == -3.0) and np.all(nms == -3.0) and ratio.value == -3.0 and np.all(lf == -3.0) and n_w.value == -3, what

    assert points() == 0 and n_pts.value >= 0 and ratio.value == 0.16 and not np.any(rank[:19] == -3.0)      # the arguments as they are: accepted
    pts[:] = -3.0; rank[:] = -3.0; nms[:] = -3.0; n_pts.value = -3; ratio.value = -3.0
    rejected("a null context", points(ctx=None), "context")
    rejected("samples without their array", points(gyro=None), "samples")
    rejected("a negative sample count", points(s=-1), "negative")
    rejected("a negative trim count", points(n_trim=-1), "negative")
    rejected("trim ranges without their array", points(trim=None), "trim")
    rejected("a null points array", points(p=None), "points_ms")
    rejected("a null point count", points(n=None), "n_points")
    rejected("no target", points(target=0), "target_sync_points")
    rejected("a negative target", points(target=-2), "target_sync_points")
    rejected("too many targets", points(target=abi.SYNC_OPTIM_TARGET_MAX + 1), "target_sync_points")
    for bad in (float("nan"), float("inf"), 0.0, -100.0):
        rejected("sample_rate %r" % bad, points(rate=bad), "sample_rate")
    rejected("a rate below the smallest fft_size", points(rate=15.4), "fft_size")
    rejected("a rate above the largest fft_size", points(rate=8192.5), "fft_size")
    rejected("too many samples", points(s=abi.SYNC_OPTIM_SAMPLES_MAX + 1), "samples", "at most")
    rejected("too many trim ranges", points(n_trim=abi.SYNC_OPTIM_TRIM_MAX + 1), "trim", "at most")
    rank_call = lambda **kw: be.lib.gfw_sync_optim_rank(kw.get("ctx", be.ctx), kw.get("gyro", g.ctypes.data), kw.get("s", 400), kw.get("rate", 100.0), lf.ctypes.data, None, None, None, C.addressof(n_w), 0)
    rejected("rank: a null context", rank_call(ctx=None), "context")
    rejected("rank: samples without their array", rank_call(gyro=None), "samples")
    rejected("rank: a NaN rate", rank_call(rate=float("nan")), "sample_rate")
    rejected("rank: a rate above the largest fft_size", rank_call(rate=9000.0), "fft_size")
    rejected("rank: too many samples", rank_call(s=abi.SYNC_OPTIM_SAMPLES_MAX + 1), "at most")
    assert rank_call() == 0 and n_w.value == 19 and not np.any(lf[:19] == -3.0) and np.all(lf[19:] == -3.0)


def test_the_python_mirror_end_to_end_on_the_200_hz_planted_clip(be):
    """OptimSync.new from raw samples (with a few missing gyro values in the quiet lead-in), .run on the device: the statement's points"""
    g, centres = S.planted_clip(200.0, 60.0)
    raw = [(i * 5.0, None if i in (3, 4, 50) else tuple(g[:, i])) for i in range(g.shape[1])]
    o = SY.OptimSync.new(raw)
    assert SY.OptimSync.new([]) is None
    want_g, want_rate = S.resample([t for t, _ in raw], [(0.0, 0.0, 0.0) if v is None else v for _, v in raw], [0 if v is None else 1 for _, v in raw])
    assert o.sample_rate == want_rate and S.same_bits(o.gyro, want_g) and S.fft_size(o.sample_rate) == 200
    pts, rank, ratio = o.run(4, [(0.0, 60.0)], be)
    assert warp.last_backend() == "sync_optim_points"
    s = S.run_f32(o.gyro, o.sample_rate, 4, [(0.0, 60.0)])
    assert S.same_bits(pts, s["points"]) and S.same_bits(rank, s["rank"]) and ratio == s["ratio"]
    lit = S.run_literal(o.gyro, o.sample_rate, 4, [(0.0, 60.0)])
    assert S.same_bits(pts, lit["points"]) and len(pts) == 4
    for c in centres:
        assert np.min(np.abs(pts - c * 1000.0)) <= 2.0 * 16.0 / o.sample_rate * 1000.0
