"""gfw_pose_almeida on the MI355X: Almeida pose estimation of all frame pairs in one device call, against the f32 statement (tests/_posestmt.py).  The arithmetic is
one rounding per operator on both sides and every sum is the reference's sequential fold, so every comparison is bit for bit: no tolerance.  The shapes are the
interpreter tier's (tests/_posecase.SPECS, the statement's results shared with tests/test_emu_pose.py); one case has the default size (200 rounds x 200 points)."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as S, warp
import _pairbase as PB
import _posecase as PC
import _posestmt as PS

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT


def backend_for(cam):
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    return warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))


def run(be, c, **kw):
    return be.pose_almeida(c.cam.kp, PC.cfg_of(c.cam), c.pairs, c.triples, c.samples, **kw)


@pytest.mark.parametrize("name", sorted(PC.SPECS))
def test_the_device_equals_the_statement_to_the_bit(name):
    c = PC.case(name)
    be = backend_for(c.cam)
    PC.assert_equal_to_statement(run(be, c, rounds=True), c.statement, name)
    assert warp.last_backend() == "pose_almeida"
    PC.assert_equal_to_statement(run(be, c), c.statement[:3], name + " without round outputs")
    for i in (1, len(c.pairs) - 1):                                                   # a pair equals its own single-pair call
        one = be.pose_almeida(c.cam.kp, PC.cfg_of(c.cam), c.pairs[i:i + 1], c.triples[i:i + 1], None if c.samples is None else c.samples[i:i + 1], rounds=True)
        PC.assert_equal_to_statement(one, [a[i:i + 1] for a in c.statement], "%s pair %d alone" % (name, i))
    be.close()


def device_outputs(n, iters):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((n, 4), -7.0, dtype=torch.float32, device=dev), torch.full((n, 3, 3), -7.0, dtype=torch.float64, device=dev),
            torch.full((n, 2), -7, dtype=torch.int32, device=dev), torch.full((n, iters), -7, dtype=torch.int32, device=dev),
            torch.full((n, iters, 4), -7.0, dtype=torch.float32, device=dev))


def test_host_and_device_outputs_agree():
    import torch
    c = PC.case("sony-stretch-r7")
    be = backend_for(c.cam)
    outs = device_outputs(len(c.pairs), c.cam.num_iters)
    torch.cuda.synchronize()
    assert run(be, c, out_ptrs=tuple(o.data_ptr() for o in outs)) is None
    PC.assert_equal_to_statement([o.cpu().numpy() for o in outs], c.statement, "device outputs")
    outs = device_outputs(len(c.pairs), c.cam.num_iters)
    torch.cuda.synchronize()
    assert run(be, c, out_ptrs=tuple(o.data_ptr() for o in outs[:3]) + (None, None)) is None
    PC.assert_equal_to_statement([o.cpu().numpy() for o in outs[:3]], c.statement[:3], "device outputs without rounds")
    assert (outs[3].cpu().numpy() == -7).all()
    be.close()


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots, other data each time, queued without waiting"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [PC.case(n) for n in ("fisheye-r7", "fisheye-r65-lists", "fisheye-r64-lists")]
    be = backend_for(cases[0].cam)
    outs = [device_outputs(len(c.pairs), c.cam.num_iters) for c in cases]
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for c, o in zip(cases, outs):
        run(be, c, out_ptrs=tuple(t.data_ptr() for t in o))
    be.synchronize()
    for c, o in zip(cases, outs):
        PC.assert_equal_to_statement([t.cpu().numpy() for t in o], c.statement, c.name + " queued")
    be.close()


def test_one_call_of_the_default_size():
    """a pair of 200 points, 200 rounds, 1000 samples (every list the whole pair, shuffled), on a pinhole camera with a planted rotation and 30 % outliers"""
    cam = PS.Camera(PC.pinhole_clip(), (960, 540))
    assert (cam.num_iters, cam.num_samples) == (200, 1000)
    a, b, R, clean = PC.plant_f64(cam, 200, (1.5, -2.5, 0.7), 0.3, 31)
    triples, samples = warp.pose_draws(7, [200], 200, 1000)
    want = PS.estimate(cam, [(a, b)], triples, samples)
    be = backend_for(cam)
    got = be.pose_almeida(cam.kp, PC.cfg_of(cam), [(a, b)], triples, samples, rounds=True)
    PC.assert_equal_to_statement(got, want, "default size")
    assert got[2][0, 0] == int(clean.sum())
    d = np.asarray(got[1][0]) - R
    assert 2.0 * np.arcsin(np.linalg.norm(d) / (2.0 * np.sqrt(2.0))) <= 0.05 / cam.K[0, 0]
    be.close()


def test_no_pairs_succeed_and_write_nothing():
    c = PC.case("fisheye-r1")
    be = backend_for(c.cam)
    quats, rot, best = be.pose_almeida(c.cam.kp, PC.cfg_of(c.cam), [], np.zeros((0, 1, 3), dtype=np.int32))
    assert quats.shape == (0, 4) and rot.shape == (0, 3, 3) and best.shape == (0, 2)
    be.close()


def raw(be, kp, cfg, first, pa, pb, n, tr, sf, sm, outs):
    p = lambda a: None if a is None else a.ctypes.data
    return be.lib.gfw_pose_almeida(be.ctx, C.byref(kp), C.byref(cfg), p(first), p(pa), p(pb), n, p(tr), p(sf), p(sm), *[p(o) for o in outs], 0)


def test_every_rejection_names_the_pair_and_leaves_the_outputs_untouched():
    c = PC.case("fisheye-r64-lists")
    cam = c.cam
    be = backend_for(cam)
    first, pa, pb = warp.Backend._pose_pairs(c.pairs)
    n, iters = len(c.pairs), cam.num_iters
    tr = np.ascontiguousarray(c.triples, dtype=np.int32)
    lists = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in c.samples]
    sf = np.zeros(n + 1, dtype=np.int32)
    sf[1:] = np.cumsum([len(s) for s in lists])
    sm = np.concatenate(lists)
    outs = [np.full((n, 4), -7.0, dtype=np.float32), np.full((n, 9), -7.0), np.full((n, 2), -7, dtype=np.int32), np.full((n, iters), -7, dtype=np.int32),
            np.full((n, iters, 4), -7.0, dtype=np.float32)]

    def refused(text, kp=None, cfg=None, first_=first, n_=n, tr_=tr, sf_=sf, sm_=sm):
        rc = raw(be, kp or cam.kp, cfg or PC.cfg_of(cam), first_, pa, pb, n_, tr_, sf_, sm_, outs)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert (outs[0] == -7.0).all() and (outs[1] == -7.0).all() and (outs[2] == -7).all() and (outs[3] == -7).all() and (outs[4] == -7.0).all()

    assert raw(be, cam.kp, PC.cfg_of(cam), first, pa, pb, n, tr, sf, sm, outs) == 0     # the arguments as they are succeed ..
    PC.assert_equal_to_statement([outs[0], outs[1].reshape(n, 3, 3)] + outs[2:], c.statement, "raw call")
    for o in outs:
        o[...] = -7                                                                  # .. and every variation below is refused
    refused("negative count", n_=-1)
    cfg = PC.cfg_of(cam); cfg.num_iters = -1
    refused("negative count", cfg=cfg)
    cfg = PC.cfg_of(cam); cfg.num_samples = -1
    refused("negative count", cfg=cfg)
    cfg = PC.cfg_of(cam); cfg.num_iters = abi.POSE_ROUNDS_MAX + 1
    refused("at most 1024", cfg=cfg)
    refused("pair 1: pair_first descends", first_=np.array([0, 12, 5], dtype=np.int32))
    refused("pair 0: pair_first -1 is negative", first_=np.array([-1, 12, 77], dtype=np.int32))
    refused("pair 0: 4097 points", first_=np.array([0, 4097, 4100], dtype=np.int32))
    t = tr.copy(); t[1, 5] = (3, 65, 4)
    refused("pair 1: round 5 draws (3, 65, 4) outside its 65 points", tr_=t)
    t = tr.copy(); t[0, 63] = (-1, 2, 4)
    refused("pair 0: round 63", tr_=t)
    t = tr.copy(); t[0, 2] = (4, 7, 4)
    refused("pair 0: round 2 draws a point twice", tr_=t)
    s = sm.copy(); s[sf[1] + 63 * 40 + 39] = 65
    refused("pair 1: sample 65 of round 63", sm_=s)
    refused("pair 1: 65 points but num_samples 40", sf_=None, sm_=None)
    refused("pair 0:", sf_=np.array([0, 12 * 64 - 1, 12 * 64 - 1 + 40 * 64], dtype=np.int32))
    for flag in (abi.FLAG_HAS_IBIS_DATA, abi.FLAG_HAS_MESH_DATA, abi.FLAG_HAS_FPD_DATA):
        kp = cam.kp.copy(); kp.flags |= flag
        refused("does not cover", kp=kp)
    kp = cam.kp.copy(); kp.f[0] = kp.f[0] + 1.0
    refused("not the f32 cast of camera_matrix", kp=kp)
    kp = cam.kp.copy(); kp.c[1] = kp.c[1] + 0.5
    refused("not the f32 cast of camera_matrix", kp=kp)
    cfg = PC.cfg_of(cam); cfg.reserved = 1
    refused("reserved", cfg=cfg)
    cfg = PC.cfg_of(cam); cfg.flow_width = 0
    refused("bad pose configuration", cfg=cfg)
    be.close()


def test_the_python_mirror_end_to_end_equals_the_statement():
    """synchronization.estimate_poses_almeida: None pairs dropped, the library's draws for the seed, rotation / quaternion / euler per pair — and estimated_gyro of them"""

    class Params:
        pass
    c = PC.case("fisheye-r7")
    cam = c.cam
    cp = Params()
    cp.lens, cp.width, cp.height, cp.output_width, cp.output_height = cam.clip.lens, cam.video[0], cam.video[1], cam.video[0], cam.video[1]
    cp.digital_lens_params, cp.light_refraction_coefficient, cp.scaled_fps = [], 1.0, 59.94
    pairs = [None] + list(c.pairs[4:8]) + [None]
    be = backend_for(cam)
    got = SY.estimate_poses_almeida(cp, pairs, be, seed=99, flow_size=cam.flow, every_nth_frame=2, num_iters=7)
    live = [p for p in pairs if p is not None]
    triples, samples = warp.pose_draws(99, [len(a) for a, _ in live], 7, 1000)
    quats, rot, best, _, _ = PS.estimate(cam, live, triples, samples)
    assert got[0] is None and got[-1] is None
    for k, r in enumerate(got[1:-1]):
        assert r["quat"].tobytes() == quats[k].tobytes() and r["rotation"].tobytes() == rot[k].tobytes() and (r["inliers"], r["round"]) == tuple(best[k])
        assert r["euler"] == tuple(SY.scaled_axis(rot[k]) * (59.94 / 2.0)) and r["quat"][0] != 1.0
    gyro = SY.estimated_gyro({1000000 + 33367 * i: (r and r["euler"]) for i, r in enumerate(got)}, 59.94)
    assert len(gyro) == 4 and all(t > 1000.0 and len(g) == 3 for t, g in gyro.values())
    be.close()


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged as given and the points from the arrays' start (tests/_pairbase.py)"""
    c = PB.almeida()
    be = backend_for(c.cam)
    quats, _, best, ri, _ = PB.assert_base_does_not_matter(lambda: run(be, c, rounds=True), "pose_almeida")
    be.close()
    assert best[1, 0] >= 3 and quats[1, 0] != 1.0 and ri.shape == (2, 4)                   # the fit, the count and the pick ran
