"""gfw_pose_essential on the MI355X: essential-matrix pose estimation of all frame pairs in one device call, against the f64 statement (tests/_posessstmt.py).  The
arithmetic is one rounding per operator on both sides (+ - * / sqrt in f64) and every sum is folded in list order, so every comparison is bit for bit: no
tolerance; a NaN is a NaN.  The shapes are the interpreter tier's (tests/_posesscase.SPECS, the statement's results shared with tests/test_emu_pose_essential.py).
The C++ mirror's end-to-end run is tests/test_cpp_pose_essential.py's."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as S, warp
import _pairbase as PB
import _posesscase as EC
import _posessstmt as ES

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT


def backend_for(cam):
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    return warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))


def run(be, c, **kw):
    return be.pose_essential(c.cam.kp, EC.cfg_of(c.cam), c.pairs, c.octets, **kw)


@pytest.mark.parametrize("name", sorted(EC.SPECS))
def test_the_device_equals_the_statement_to_the_bit(name):
    c = EC.case(name)
    be = backend_for(c.cam)
    EC.assert_equal_to_statement(run(be, c, rounds=True), c.statement, name)
    assert warp.last_backend() == "pose_essential"
    EC.assert_equal_to_statement(run(be, c), c.statement[:4], name + " without round outputs")
    for i in (0, len(c.pairs) - 1):                                                   # a pair equals its own single-pair call
        one = be.pose_essential(c.cam.kp, EC.cfg_of(c.cam), c.pairs[i:i + 1], c.octets[i:i + 1], rounds=True)
        EC.assert_equal_to_statement(one, [a[i:i + 1] for a in c.statement], "%s pair %d alone" % (name, i))
    be.close()


def device_outputs(n, iters):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((n, 4), -7.0, dtype=torch.float32, device=dev), torch.full((n, 3, 3), -7.0, dtype=torch.float64, device=dev),
            torch.full((n, 9), -7.0, dtype=torch.float64, device=dev), torch.full((n, 4), -7, dtype=torch.int32, device=dev),
            torch.full((n, iters), -7, dtype=torch.int32, device=dev), torch.full((n, iters, 9), -7.0, dtype=torch.float64, device=dev))


def test_host_and_device_outputs_agree():
    import torch
    c = EC.case("sony-stretch-r7")
    be = backend_for(c.cam)
    outs = device_outputs(len(c.pairs), c.cam.num_iters)
    torch.cuda.synchronize()
    assert run(be, c, out_ptrs=tuple(o.data_ptr() for o in outs)) is None
    EC.assert_equal_to_statement([o.cpu().numpy() for o in outs], c.statement, "device outputs")
    outs = device_outputs(len(c.pairs), c.cam.num_iters)
    torch.cuda.synchronize()
    assert run(be, c, out_ptrs=tuple(o.data_ptr() for o in outs[:4]) + (None, None)) is None
    EC.assert_equal_to_statement([o.cpu().numpy() for o in outs[:4]], c.statement[:4], "device outputs without rounds")
    assert (outs[4].cpu().numpy() == -7).all() and (outs[5].cpu().numpy() == -7.0).all()
    be.close()


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots (two), other data each time, queued without waiting"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [EC.case(n) for n in ("fisheye-r7", "fisheye-r65", "fisheye-r64")]
    be = backend_for(cases[0].cam)
    outs = [device_outputs(len(c.pairs), c.cam.num_iters) for c in cases]
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for c, o in zip(cases, outs):
        run(be, c, out_ptrs=tuple(t.data_ptr() for t in o))
    be.synchronize()
    for c, o in zip(cases, outs):
        EC.assert_equal_to_statement([t.cpu().numpy() for t in o], c.statement, c.name + " queued")
    be.close()


def test_no_pairs_succeed_and_write_nothing():
    c = EC.case("fisheye-r1")
    be = backend_for(c.cam)
    quats, rot, ess, best = be.pose_essential(c.cam.kp, EC.cfg_of(c.cam), [], np.zeros((0, 1, 8), dtype=np.int32))
    assert quats.shape == (0, 4) and rot.shape == (0, 3, 3) and ess.shape == (0, 9) and best.shape == (0, 4)
    be.close()


def raw(be, kp, cfg, first, pa, pb, n, oc, outs):
    p = lambda a: None if a is None else a.ctypes.data
    return be.lib.gfw_pose_essential(be.ctx, C.byref(kp), C.byref(cfg), p(first), p(pa), p(pb), n, p(oc), *[p(o) for o in outs], 0)


def test_every_rejection_names_the_pair_and_leaves_the_outputs_untouched():
    c = EC.case("fisheye-r64")
    cam = c.cam
    be = backend_for(cam)
    first, pa, pb = warp.Backend._pose_pairs(c.pairs)
    n, iters = len(c.pairs), cam.num_iters
    oc = np.ascontiguousarray(c.octets, dtype=np.int32)
    outs = [np.full((n, 4), -7.0, dtype=np.float32), np.full((n, 9), -7.0), np.full((n, 9), -7.0), np.full((n, 4), -7, dtype=np.int32),
            np.full((n, iters), -7, dtype=np.int32), np.full((n, iters, 9), -7.0)]

    def refused(text, kp=None, cfg=None, first_=first, n_=n, oc_=oc, pa_=pa, outs_=None):
        rc = raw(be, kp or cam.kp, cfg or EC.cfg_of(cam), first_, pa_, pb, n_, oc_, outs_ or outs)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert all((o == -7).all() for o in outs)

    assert raw(be, cam.kp, EC.cfg_of(cam), first, pa, pb, n, oc, outs) == 0              # the arguments as they are succeed ..
    EC.assert_equal_to_statement([outs[0], outs[1].reshape(n, 3, 3)] + outs[2:], c.statement, "raw call")
    for o in outs:
        o[...] = -7                                                                  # .. and every variation below is refused
    refused("negative count", n_=-1)
    cfg = EC.cfg_of(cam); cfg.num_iters = -1
    refused("negative count", cfg=cfg)
    cfg = EC.cfg_of(cam); cfg.num_iters = abi.POSE_ROUNDS_MAX + 1
    refused("at most 1024", cfg=cfg)
    refused("at most 65535", n_=abi.POSE_PAIRS_MAX + 1)
    refused("pair 1: pair_first descends", first_=np.array([0, 12, 5], dtype=np.int32))
    refused("pair 0: pair_first -1 is negative", first_=np.array([-1, 12, 77], dtype=np.int32))
    refused("pair 0: 4097 points", first_=np.array([0, 4097, 4100], dtype=np.int32))
    refused("without pair_first", first_=None)
    refused("without points_a / points_b", pa_=None)
    refused("rounds without octets", oc_=None)
    refused("a null quats / rotations / essential / best array", outs_=[outs[0], None] + outs[2:])
    o = oc.copy(); o[1, 5, 3] = 65
    refused("pair 1: round 5 draws 65 outside its 65 points", oc_=o)
    o = oc.copy(); o[0, 63, 0] = -1
    refused("pair 0: round 63", oc_=o)
    o = oc.copy(); o[0, 2, 6] = o[0, 2, 1]
    refused("pair 0: round 2 draws a point twice", oc_=o)
    for flag in (abi.FLAG_HAS_IBIS_DATA, abi.FLAG_HAS_MESH_DATA, abi.FLAG_HAS_FPD_DATA):
        kp = cam.kp.copy(); kp.flags |= flag
        refused("does not cover", kp=kp)
    kp = cam.kp.copy(); kp.f[0] = kp.f[0] + 1.0
    refused("not the f32 cast of camera_matrix", kp=kp)
    kp = cam.kp.copy(); kp.c[1] = kp.c[1] + 0.5
    refused("not the f32 cast of camera_matrix", kp=kp)
    cfg = EC.cfg_of(cam); cfg.reserved[1] = 1
    refused("reserved", cfg=cfg)
    cfg = EC.cfg_of(cam); cfg.flow_width = 0
    refused("bad pose configuration", cfg=cfg)
    cfg = EC.cfg_of(cam); cfg.inlier_threshold = -1e-9
    refused("bad pose configuration", cfg=cfg)
    cfg = EC.cfg_of(cam); cfg.inlier_threshold = float("nan")
    refused("bad pose configuration", cfg=cfg)
    cfg = EC.cfg_of(cam); cfg.min_front = -1
    refused("bad pose configuration", cfg=cfg)
    o = oc.copy(); o[...] = 99                                                       # octets of pairs under 8 points are ignored
    small = [np.full((1, 4), -7.0, dtype=np.float32), np.full((1, 9), -7.0), np.full((1, 9), -7.0), np.full((1, 4), -7, dtype=np.int32), None, None]
    assert raw(be, cam.kp, EC.cfg_of(cam), np.array([0, 7], dtype=np.int32), pa, pb, 1, o, small) == 0
    assert small[3].tolist() == [[0, 0, 0, 0]] and small[0].tolist() == [[1.0, 0.0, 0.0, 0.0]]
    be.close()


def test_frames_on_the_device_to_rotations_with_the_points_copied_back_between_the_calls():
    """frames in device memory -> flow_pyrlk with device outputs -> the compacted arrays COPIED TO THE HOST (gfw_pose_essential stages its points from host memory) ->
    pose_essential: equal to the CPU chain's (statement of the flow, then statement of the pose) to the bit"""
    import torch
    import _flowcase as FC
    from test_gpu_flow import device_outputs as flow_outputs, ORDER
    c = FC.case("odd-384x216")
    cam = ES.Camera(c.cam.clip, c.cam.flow, num_iters=24)
    be = backend_for(cam)
    d_frames = torch.from_numpy(c.frames).to(torch.device("cuda", 0))
    outs = flow_outputs(3 * FC.N_FEATURES, 3, 3, warp.flow_grid_nodes(c.width, c.height))
    torch.cuda.synchronize()
    ptrs = [outs[k].data_ptr() for k in ORDER]
    ptrs[2] = ptrs[3] = ptrs[4] = None
    be.flow_pyrlk(d_frames.data_ptr(), c.width, FC.PAIRS, c.features, out_ptrs=tuple(ptrs), shape=c.frames.shape)
    assert warp.last_backend() == "flow_pyrlk"
    first = outs["pair_first"].cpu().numpy()
    a, b = outs["points_a"].cpu().numpy(), outs["points_b"].cpu().numpy()
    pairs = [(a[first[p]:first[p + 1]], b[first[p]:first[p + 1]]) for p in range(3)]
    s = c.statement
    want_pairs = [(s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]], s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]]) for p in range(3)]
    octets = EC.draws([len(x) for x, _ in want_pairs], cam.num_iters, 77)
    got = be.pose_essential(cam.kp, EC.cfg_of(cam), pairs, octets)
    assert warp.last_backend() == "pose_essential"
    EC.assert_equal_to_statement(got, ES.estimate(cam, want_pairs, octets)[:4], "frames to rotations")
    be.close()


class Params:
    pass


def compute_params(cam):
    cp = Params()
    cp.lens, cp.width, cp.height, cp.output_width, cp.output_height = cam.clip.lens, cam.video[0], cam.video[1], cam.video[0], cam.video[1]
    cp.digital_lens_params, cp.light_refraction_coefficient, cp.scaled_fps = [], 1.0, 59.94
    return cp


def test_the_python_mirror_end_to_end_equals_the_statement():
    """synchronization.estimate_poses_essential: None pairs dropped, the library's draws for the seed, rotation / quaternion / euler per pair, None where no rotation
    is found — and estimated_gyro of them; estimate_poses dispatches methods 0 and 2 to it, 1 and unknown values to Almeida, and refuses 3"""
    c = EC.case("fisheye-r7")
    cam = c.cam
    cp = compute_params(cam)
    pairs = [None] + list(c.pairs[2:7]) + [None]
    be = backend_for(cam)
    got = SY.estimate_poses_essential(cp, pairs, be, seed=99, flow_size=cam.flow, every_nth_frame=2, num_iters=7)
    assert warp.last_backend() == "pose_essential"
    live = [p for p in pairs if p is not None]
    octets = warp.pose_draws_k(99, [len(a) for a, _ in live], 7, 8)
    quats, rot, ess, best, _, _ = ES.estimate(cam, live, octets)
    assert got[0] is None and got[-1] is None and best[:, 3].any() and not best[:, 3].all()
    for k, r in enumerate(got[1:-1]):
        if not best[k, 3]:
            assert r is None
            continue
        assert r["quat"].tobytes() == quats[k].tobytes() and r["rotation"].tobytes() == rot[k].tobytes()
        assert (r["inliers"], r["round"], r["front"]) == tuple(best[k, :3])
        assert r["euler"] == tuple(SY.scaled_axis(rot[k]) * (59.94 / 2.0)) and r["quat"][0] != 1.0
    gyro = SY.estimated_gyro({1000000 + 33367 * i: (r and r["euler"]) for i, r in enumerate(got)}, 59.94)
    assert len(gyro) == int(best[:, 3].sum()) and all(t > 1000.0 and len(g) == 3 for t, g in gyro.values())
    for method in (0, 2):
        again = SY.estimate_poses(method, cp, pairs, be, seed=99, flow_size=cam.flow, every_nth_frame=2, num_iters=7)
        assert warp.last_backend() == "pose_essential"
        assert [r and r["rotation"].tobytes() for r in again] == [r and r["rotation"].tobytes() for r in got]
    for method in (1, 7):
        other = SY.estimate_poses(method, cp, pairs, be, seed=99, flow_size=cam.flow, every_nth_frame=2, num_iters=7)
        assert warp.last_backend() == "pose_almeida" and other[0] is None and "front" not in other[1]
    with pytest.raises(NotImplementedError):
        SY.estimate_poses(3, cp, pairs, be)
    be.close()


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged as given and the points from the arrays' start (tests/_pairbase.py)"""
    c = PB.essential()
    be = backend_for(c.cam)
    _, _, _, _, ri, rf = PB.assert_base_does_not_matter(lambda: run(be, c, rounds=True), "pose_essential")
    be.close()
    assert ri.shape == (2, 4) and rf.any() and ri.any()                                    # the fits and the counts ran
