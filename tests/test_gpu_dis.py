"""gfw_flow_dis on the MI355X: the DIS dense optical flow of all frame pairs in one device call, against the fixed-point statement (tests/_disstmt.py).  Every sum
over a patch is an integer and every f32 operation is one rounding on both sides, so every comparison is bit for bit: no tolerance.  The shapes are the interpreter
tier's (tests/_discase.CONFIGS: the three scenes at both finest scales; the statement's results shared with tests/test_emu_dis.py)."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as S, warp
import _discase as DC
import _posecase as PC
import _posestmt as PS

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT
ORDER = ("grid_points", "grid_counts", "flow", "pair_first", "points_a", "points_b")


def backend_for(cam):
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    return warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))


def device_outputs(c, n_pairs, finest):
    import torch
    dev = torch.device("cuda", 0)
    full = lambda shape, v, t: torch.full(shape, v, dtype=t, device=dev)
    nodes = warp.flow_grid_nodes(c.width, c.height)
    return {"grid_points": full((len(c.frames), nodes, 2), -7.0, torch.float32), "grid_counts": full((len(c.frames),), -7, torch.int32),
            "flow": full((n_pairs, c.height >> finest, c.width >> finest, 2), -7.0, torch.float32), "pair_first": full((n_pairs + 1,), -7, torch.int32),
            "points_a": full((n_pairs * nodes, 2), -7.0, torch.float32), "points_b": full((n_pairs * nodes, 2), -7.0, torch.float32)}


def fetch(outs):
    got = {k: outs[k].cpu().numpy() for k in ORDER}
    total = int(got["pair_first"][-1])
    assert (got["points_a"][total:] == -7.0).all() and (got["points_b"][total:] == -7.0).all()      # only the returned entries are written
    got["points_a"], got["points_b"] = got["points_a"][:total], got["points_b"][:total]
    return got


@pytest.mark.parametrize("name,finest", DC.CONFIGS)
def test_the_device_equals_the_statement_to_the_bit_from_host_and_device_memory(name, finest):
    """all four combinations: host and device frames x host and device outputs"""
    import torch
    c = DC.case(name)
    want = DC.statement(name, finest)[0]
    be = backend_for(c.cam)
    d_frames = torch.from_numpy(c.frames).to(torch.device("cuda", 0))
    DC.assert_equal_to_statement(be.flow_dis(c.frames, c.width, c.pairs, finest, flow=True), want, "%s finest %d: host frames, host outputs" % (name, finest))
    assert warp.last_backend() == "flow_dis"
    DC.assert_equal_to_statement(be.flow_dis(d_frames.data_ptr(), c.width, c.pairs, finest, flow=True, shape=c.frames.shape), want, name + ": device frames, host outputs")
    for frames, shape, what in ((c.frames, None, "host frames"), (d_frames.data_ptr(), c.frames.shape, "device frames")):
        outs = device_outputs(c, len(c.pairs), finest)
        torch.cuda.synchronize()
        nodes = warp.flow_grid_nodes(c.width, c.height)
        assert be.flow_dis(frames, c.width, c.pairs, finest, out_ptrs=tuple(outs[k].data_ptr() for k in ORDER), shape=shape) == len(c.pairs) * nodes
        DC.assert_equal_to_statement(fetch(outs), want, "%s: %s, device outputs" % (name, what))
    be.close()


def test_without_the_optional_outputs_and_a_pair_alone():
    c = DC.case("cut-200x168")
    s = DC.statement("cut-200x168", 2)[0]
    be = backend_for(c.cam)
    got = be.flow_dis(c.frames, c.width, c.pairs)
    DC.assert_equal_to_statement(got, s, "without the dense field", ("grid_points", "grid_counts", "pair_first", "points_a", "points_b"))
    one = be.flow_dis(c.frames, c.width, [c.pairs[2]], flow=True)                                    # a pair equals its own single-pair call
    assert np.array_equal(one["points_b"].view(np.uint32), s["points_b"][s["pair_first"][2]:].view(np.uint32)) and np.array_equal(one["flow"][0].view(np.uint32), s["flow"][2].view(np.uint32))
    assert one["pair_first"].tolist() == [0, s["pair_first"][3] - s["pair_first"][2]]
    got = be.flow_dis(c.frames, c.width, np.zeros((0, 2), dtype=np.int32))                          # no pairs succeed and write nothing
    assert got["pair_first"].tolist() == [0] and got["points_a"].shape == (0, 2) and (got["grid_counts"] == 0).all()
    be.close()


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots, other data each time, queued without waiting"""
    import torch
    dev = torch.device("cuda", 0)
    calls = [("cut-200x168", 2), ("odd-384x216", 2), ("exits-96x64", 1)]
    assert len(calls) == abi.DIS_RING_SLOTS + 1
    be = backend_for(DC.case(calls[0][0]).cam)
    outs = [device_outputs(DC.case(name), 3, finest) for name, finest in calls]
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for (name, finest), o in zip(calls, outs):
        c = DC.case(name)
        be.flow_dis(c.frames, c.width, c.pairs, finest, out_ptrs=tuple(o[k].data_ptr() for k in ORDER))
    be.synchronize()
    for (name, finest), o in zip(calls, outs):
        DC.assert_equal_to_statement(fetch(o), DC.statement(name, finest)[0], name + " queued")
    be.close()


def test_every_rejection_names_the_pair_or_frame_and_leaves_the_outputs_untouched():
    c = DC.case("cut-200x168")
    be = backend_for(c.cam)
    pf = np.ascontiguousarray(c.pairs, dtype=np.int32)
    nodes = warp.flow_grid_nodes(c.width, c.height)
    outs = [np.full((3, nodes, 2), -7.0, dtype=np.float32), np.full(3, -7, dtype=np.int32), np.full((3, 42, 50, 2), -7.0, dtype=np.float32),
            np.full(4, -7, dtype=np.int32), np.full((3 * nodes, 2), -7.0, dtype=np.float32), np.full((3 * nodes, 2), -7.0, dtype=np.float32)]
    p = lambda a: None if a is None else a.ctypes.data

    def call(cfg=None, frames=c.frames, n_frames=3, pf_=pf, n_pairs=3, outs_=None):
        cfg = cfg or abi.FlowDisCfg(width=c.width, height=c.height, stride=c.stride, finest_scale=2)
        return be.lib.gfw_flow_dis(be.ctx, C.byref(cfg), p(frames), 0, n_frames, p(pf_), n_pairs, *[p(o) for o in (outs_ or outs)], 0)

    def refused(text, **kw):
        rc = call(**kw)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert all((o == -7).all() for o in outs)

    assert call() == 0                                                               # the arguments as they are succeed ..
    total = int(outs[3][-1])
    DC.assert_equal_to_statement(dict(zip(ORDER, outs[:4] + [outs[4][:total], outs[5][:total]])), DC.statement("cut-200x168", 2)[0], "raw call")
    assert (outs[4][total:] == -7.0).all() and (outs[5][total:] == -7.0).all()
    for o in outs:
        o[...] = -7                                                                  # .. and every variation below is refused
    cfg = lambda **kw: abi.FlowDisCfg(**dict(dict(width=c.width, height=c.height, stride=c.stride, finest_scale=2), **kw))
    refused("negative count", n_pairs=-1)
    refused("negative count", n_frames=-1)
    refused("without pair_frames", pf_=None)
    refused("3 frames without their planes", frames=None)
    refused("a null out_pair_first", outs_=outs[:3] + [None] + outs[4:])
    refused("a null out_pair_first", outs_=outs[:5] + [None])
    refused("pair 1: frames (1, 3) outside the call's 3 frames", pf_=np.array([[0, 1], [1, 3], [0, 2]], dtype=np.int32))
    refused("pair 0: frames (-1, 1) outside", pf_=np.array([[-1, 1], [1, 2], [0, 2]], dtype=np.int32))
    refused("pair 2: frame 2 paired with itself", pf_=np.array([[0, 1], [1, 2], [2, 2]], dtype=np.int32))
    refused("frames of 256 x 24 have the coarsest scale 1, under the finest scale 2", cfg=cfg(width=256, height=24, stride=256))
    refused("frames of 200 x 8193", cfg=cfg(height=8193))
    refused("stride 199 under the width 200", cfg=cfg(stride=199))
    refused("finest_scale 3", cfg=cfg(finest_scale=3))
    refused("finest_scale 0", cfg=cfg(finest_scale=0))
    refused("variational_iters 5", cfg=cfg(variational_iters=5))
    refused("reserved", cfg=cfg(reserved=1))
    refused("4097 frames", n_frames=abi.DIS_FRAMES_MAX + 1)
    refused("65536 pairs", n_pairs=abi.DIS_PAIRS_MAX + 1)
    refused("at most 2 GiB", cfg=cfg(stride=1 << 20, height=3000))          # 3 host frames of 3 GiB each: refused unread (3000 rows: the grid stays under 4096 nodes)
    refused("the grid of a 16 x 8192 frame has 131072 nodes", cfg=cfg(width=16, height=8192, stride=16, finest_scale=1), n_frames=2, n_pairs=1)
    be.close()


def test_frames_on_the_device_to_rotations_with_the_points_copied_back_between_the_calls():
    """frames in device memory -> flow_dis with device outputs -> the points COPIED TO THE HOST (gfw_pose_almeida stages its points from host memory) ->
    pose_almeida: the rotation equals the CPU chain's (statement of the flow, then statement of the pose) to the bit, and is within 0.1 degrees of the plant
    (tests/test_dis_statement.py's bar at the reference's finest scale)"""
    import torch
    from test_pose_statement import rotation_error
    c = DC.case("odd-384x216")
    cam = c.cam
    be = backend_for(cam)
    d_frames = torch.from_numpy(c.frames).to(torch.device("cuda", 0))
    outs = device_outputs(c, 3, 2)
    torch.cuda.synchronize()
    ptrs = [outs[k].data_ptr() for k in ORDER]
    ptrs[0] = ptrs[1] = ptrs[2] = None
    be.flow_dis(d_frames.data_ptr(), c.width, c.pairs, 2, out_ptrs=tuple(ptrs), shape=c.frames.shape)
    first = outs["pair_first"].cpu().numpy()
    a, b = outs["points_a"].cpu().numpy(), outs["points_b"].cpu().numpy()
    pairs = [(a[first[p]:first[p + 1]], b[first[p]:first[p + 1]]) for p in range(3)]
    s = DC.statement("odd-384x216", 2)[0]
    want_pairs = [(s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]], s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]]) for p in range(3)]
    triples, _ = PC.draws([len(x) for x, _ in want_pairs], cam.num_iters, cam.num_samples, 77, False)
    quats, rot, best = be.pose_almeida(cam.kp, PC.cfg_of(cam), pairs, triples)
    assert warp.last_backend() == "pose_almeida"
    want = PS.estimate(cam, want_pairs, triples, None)
    PC.assert_equal_to_statement((quats, rot, best), want[:3], "frames to rotations")
    for p, (fa, fb) in enumerate(c.pairs):
        assert np.degrees(rotation_error(c.rotation(fa, fb), rot[p])) < 0.1
    be.close()


def test_the_python_mirror_returns_what_the_pose_stage_takes():
    c = DC.case("cut-200x168")
    be = backend_for(c.cam)
    for finest in DC.FINEST:
        s = DC.statement("cut-200x168", finest)[0]
        got = SY.optical_flow_dis(c.frames, c.pairs, backend=be, width=c.width, finest_scale=finest)
        for p, r in enumerate(got):
            assert np.array_equal(r[0], s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]]) and np.array_equal(r[1], s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]])
    flat = np.full((2, c.height, c.stride), 128, dtype=np.uint8)                                       # no node kept: under 10 points, None (opencv_dis.rs:126)
    assert SY.optical_flow_dis(flat, [(0, 1)], backend=be, width=c.width) == [None]
    be.close()
