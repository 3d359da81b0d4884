"""gfw_flow_pyrlk on the MI355X: pyramidal Lucas-Kanade optical flow of all frame pairs in one device call, against the fixed-point statement (tests/_flowstmt.py).
Every window sum is an integer and every f32 operation is one rounding on both sides, so every comparison is bit for bit: no tolerance.  The shapes are the
interpreter tier's (tests/_flowcase.ALL_SPECS: the analytic scenes and the out-of-level exit case; the statement's results shared with tests/test_emu_flow.py)."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as S, warp
import _flowcase as FC
import _posecase as PC
import _posestmt as PS

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT
NAMES = sorted(FC.ALL_SPECS)


def backend_for(cam):
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    return warp.Backend(pl["params"], pl["pixel_type"], cam.clip.model, cam.clip.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))


@pytest.mark.parametrize("name", NAMES)
def test_the_device_equals_the_statement_to_the_bit(name):
    c = FC.case(name)
    be = backend_for(c.cam)
    FC.assert_equal_to_statement(be.flow_pyrlk(c.frames, c.width, c.pairs, c.features, iters=True), c.statement, name)
    assert warp.last_backend() == "flow_pyrlk"
    FC.assert_equal_to_statement(be.flow_pyrlk(c.frames, c.width, c.pairs, c.features), c.statement, name + " without iters",
                                 ("next", "status", "pair_first", "points_a", "points_b"))
    s, last = c.statement, FC.raw_slices(c)[2]
    one = be.flow_pyrlk(c.frames, c.width, [c.pairs[2]], c.features, iters=True)                  # a pair equals its own single-pair call
    assert np.array_equal(one["next"].view(np.uint32), s["next"][last].view(np.uint32)) and np.array_equal(one["status"], s["status"][last])
    assert np.array_equal(one["iters"], s["iters"][last]) and np.array_equal(one["points_b"], s["points_b"][s["pair_first"][2]:])
    assert one["pair_first"].tolist() == [0, s["pair_first"][3] - s["pair_first"][2]]
    be.close()


@pytest.mark.parametrize("name", NAMES)
def test_the_grid_mode_equals_the_statement_to_the_bit(name):
    c = FC.case(name)
    be = backend_for(c.cam)
    FC.assert_equal_to_statement(be.flow_pyrlk(c.frames, c.width, c.pairs, None, iters=True), c.grid_statement, name + " grid", FC.GRID_OUTPUTS)
    assert warp.last_backend() == "flow_pyrlk"
    be.close()


def device_outputs(raw, n_pairs, n_frames, nodes):
    import torch
    dev = torch.device("cuda", 0)
    full = lambda shape, v, t: torch.full(shape, v, dtype=t, device=dev)
    return {"next": full((raw, 2), -7.0, torch.float32), "status": full((raw,), 7, torch.uint8), "iters": full((raw, 4), -7, torch.int32),
            "grid_points": full((n_frames, nodes, 2), -7.0, torch.float32), "grid_counts": full((n_frames,), -7, torch.int32),
            "pair_first": full((n_pairs + 1,), -7, torch.int32), "points_a": full((raw, 2), -7.0, torch.float32), "points_b": full((raw, 2), -7.0, torch.float32)}


ORDER = ("next", "status", "iters", "grid_points", "grid_counts", "pair_first", "points_a", "points_b")


def fetch(outs, names):
    got = {k: outs[k].cpu().numpy() for k in names}
    kept = int(got["pair_first"][-1])
    assert (got["points_a"][kept:] == -7.0).all() and (got["points_b"][kept:] == -7.0).all()      # only the kept entries are written
    got["points_a"], got["points_b"] = got["points_a"][:kept], got["points_b"][:kept]
    return got


def test_device_frames_and_device_outputs_agree_in_both_modes():
    import torch
    c = FC.case("cut-200x168")
    be = backend_for(c.cam)
    d_frames = torch.from_numpy(c.frames).to(torch.device("cuda", 0))
    nodes = warp.flow_grid_nodes(c.width, c.height)
    # the caller's features: device frames, device outputs, without the optional arrays
    outs = device_outputs(3 * FC.N_FEATURES, 3, 3, nodes)
    torch.cuda.synchronize()
    ptrs = [outs[k].data_ptr() for k in ORDER]
    ptrs[2] = ptrs[3] = ptrs[4] = None
    assert be.flow_pyrlk(d_frames.data_ptr(), c.width, FC.PAIRS, c.features, out_ptrs=tuple(ptrs), shape=c.frames.shape) == 3 * FC.N_FEATURES
    FC.assert_equal_to_statement(fetch(outs, ORDER), c.statement, "device frames and outputs", ("next", "status", "pair_first", "points_a", "points_b"))
    assert (outs["iters"].cpu().numpy() == -7).all() and warp.last_backend() == "flow_pyrlk"
    # device frames, host outputs
    FC.assert_equal_to_statement(be.flow_pyrlk(d_frames.data_ptr(), c.width, FC.PAIRS, c.features, iters=True, shape=c.frames.shape), c.statement, "device frames")
    # the grid mode: host frames, device outputs, every array
    outs = device_outputs(3 * nodes, 3, 3, nodes)
    torch.cuda.synchronize()
    assert be.flow_pyrlk(c.frames, c.width, FC.PAIRS, None, out_ptrs=tuple(outs[k].data_ptr() for k in ORDER)) == 3 * nodes
    FC.assert_equal_to_statement(fetch(outs, ORDER), c.grid_statement, "grid mode, device outputs", FC.GRID_OUTPUTS)
    be.close()


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots, other data each time, queued without waiting"""
    import torch
    dev = torch.device("cuda", 0)
    calls = [(FC.case("cut-200x168"), True), (FC.case("odd-384x216"), True), (FC.case("cut-200x168"), False)]
    assert len(calls) == abi.FLOW_RING_SLOTS + 1
    be = backend_for(calls[0][0].cam)
    outs = []
    for c, feats in calls:
        nodes = warp.flow_grid_nodes(c.width, c.height)
        outs.append(device_outputs(3 * (FC.N_FEATURES if feats else nodes), 3, 3, nodes))
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for (c, feats), o in zip(calls, outs):
        be.flow_pyrlk(c.frames, c.width, FC.PAIRS, c.features if feats else None, out_ptrs=tuple(o[k].data_ptr() for k in ORDER))
    be.synchronize()
    for (c, feats), o in zip(calls, outs):
        FC.assert_equal_to_statement(fetch(o, ORDER), c.statement if feats else c.grid_statement, c.name + " queued", FC.OUTPUTS if feats else FC.GRID_OUTPUTS)
    be.close()


def test_no_pairs_succeed_and_write_nothing():
    c = FC.case("cut-200x168")
    be = backend_for(c.cam)
    got = be.flow_pyrlk(c.frames, c.width, np.zeros((0, 2), dtype=np.int32), c.features)
    assert got["next"].shape == (0, 2) and got["pair_first"].tolist() == [0] and got["points_a"].shape == (0, 2)
    be.close()


def test_every_rejection_names_the_pair_or_frame_and_leaves_the_outputs_untouched():
    c = FC.case("cut-200x168")
    be = backend_for(c.cam)
    ff, ft = warp.Backend._flow_features(c.features)
    pf = np.ascontiguousarray(FC.PAIRS, dtype=np.int32)
    raw = 3 * FC.N_FEATURES
    outs = [np.full((raw, 2), -7.0, dtype=np.float32), np.full(raw, 7, dtype=np.uint8), np.full((raw, 4), -7, dtype=np.int32), None, None,
            np.full(4, -7, dtype=np.int32), np.full((raw, 2), -7.0, dtype=np.float32), np.full((raw, 2), -7.0, dtype=np.float32)]
    p = lambda a: None if a is None else a.ctypes.data

    def call(cfg=None, frames=c.frames, n_frames=3, pf_=pf, n_pairs=3, ff_=ff, ft_=ft, outs_=None):
        cfg = cfg or abi.FlowPyrLKCfg(width=c.width, height=c.height, stride=c.stride, point_mode=0)
        return be.lib.gfw_flow_pyrlk(be.ctx, C.byref(cfg), p(frames), 0, n_frames, p(pf_), n_pairs, p(ff_), p(ft_), *[p(o) for o in (outs_ or outs)], 0)

    def refused(text, **kw):
        rc = call(**kw)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert all((o == (7 if o.dtype == np.uint8 else -7)).all() for o in outs if o is not None)

    assert call() == 0                                                               # the arguments as they are succeed ..
    kept = int(outs[5][-1])
    FC.assert_equal_to_statement({"next": outs[0], "status": outs[1], "iters": outs[2], "pair_first": outs[5], "points_a": outs[6][:kept], "points_b": outs[7][:kept]},
                                 c.statement, "raw call")
    assert (outs[6][kept:] == -7.0).all() and (outs[7][kept:] == -7.0).all()
    for o in outs:
        if o is not None:
            o[...] = 7 if o.dtype == np.uint8 else -7                                # .. and every variation below is refused
    cfg = lambda **kw: abi.FlowPyrLKCfg(**dict(dict(width=c.width, height=c.height, stride=c.stride, point_mode=0), **kw))
    refused("negative count", n_pairs=-1)
    refused("negative count", n_frames=-1)
    refused("without pair_frames", pf_=None)
    refused("3 frames without their planes", frames=None)
    refused("point mode 0 without features", ff_=None)
    refused("point mode 0 without features", ft_=None)
    refused("a null next / status", outs_=[None] + outs[1:])
    refused("a null next / status", outs_=outs[:5] + [None] + outs[6:])
    refused("frame 1: feat_first descends (60 after 70)", ff_=np.array([0, 70, 60, 210], dtype=np.int32))
    refused("frame 0: feat_first -1 is negative", ff_=np.array([-1, 70, 140, 210], dtype=np.int32))
    refused("frame 2: 4097 features", ff_=np.array([0, 70, 140, 140 + 4097], dtype=np.int32))
    refused("pair 1: frames (1, 3) outside the call's 3 frames", pf_=np.array([[0, 1], [1, 3], [0, 2]], dtype=np.int32))
    refused("pair 0: frames (-1, 1) outside", pf_=np.array([[-1, 1], [1, 2], [0, 2]], dtype=np.int32))
    refused("pair 2: frame 2 paired with itself", pf_=np.array([[0, 1], [1, 2], [2, 2]], dtype=np.int32))
    refused("frames of 23 x 168", cfg=cfg(width=23))
    refused("frames of 200 x 8193", cfg=cfg(height=8193))
    refused("stride 199 under the width 200", cfg=cfg(stride=199))
    refused("point mode 2", cfg=cfg(point_mode=2))
    refused("reserved", cfg=cfg(reserved=1))
    refused("4097 frames", n_frames=abi.FLOW_FRAMES_MAX + 1)
    refused("65536 pairs", n_pairs=abi.FLOW_PAIRS_MAX + 1)
    refused("at most 2 GiB", cfg=cfg(stride=1 << 20, height=8192))          # 3 host frames of 8 GiB each: refused unread
    refused("the grid of a 24 x 8192 frame has 196608 nodes", cfg=cfg(width=24, height=8192, stride=24, point_mode=1), n_frames=2, n_pairs=1)
    be.close()


def test_frames_on_the_device_to_rotations_with_the_points_copied_back_between_the_calls():
    """frames in device memory -> flow_pyrlk with device outputs -> the compacted arrays COPIED TO THE HOST (gfw_pose_almeida stages its points from host memory:
    the device outputs cannot yet be consumed on the device) -> pose_almeida: the rotation equals the CPU chain's (statement of the flow, then statement of the
    pose) to the bit, and is therefore within 0.05 degrees of the plant (tests/test_flow_statement.py)"""
    import torch
    from test_pose_statement import rotation_error
    c = FC.case("odd-384x216")
    cam = c.cam
    be = backend_for(cam)
    d_frames = torch.from_numpy(c.frames).to(torch.device("cuda", 0))
    nodes = warp.flow_grid_nodes(c.width, c.height)
    outs = device_outputs(3 * FC.N_FEATURES, 3, 3, nodes)
    torch.cuda.synchronize()
    ptrs = [outs[k].data_ptr() for k in ORDER]
    ptrs[2] = ptrs[3] = ptrs[4] = None
    be.flow_pyrlk(d_frames.data_ptr(), c.width, FC.PAIRS, c.features, out_ptrs=tuple(ptrs), shape=c.frames.shape)
    first = outs["pair_first"].cpu().numpy()                                          # (gfw_pose_almeida stages its points from host memory)
    a, b = outs["points_a"].cpu().numpy(), outs["points_b"].cpu().numpy()
    pairs = [(a[first[p]:first[p + 1]], b[first[p]:first[p + 1]]) for p in range(3)]
    s = c.statement
    want_pairs = [(s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]], s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]]) for p in range(3)]
    triples, _ = PC.draws([len(x) for x, _ in want_pairs], cam.num_iters, cam.num_samples, 77, False)
    quats, rot, best = be.pose_almeida(cam.kp, PC.cfg_of(cam), pairs, triples)
    assert warp.last_backend() == "pose_almeida"
    want = PS.estimate(cam, want_pairs, triples, None)
    PC.assert_equal_to_statement((quats, rot, best), want[:3], "frames to rotations")
    for p, (fa, fb) in enumerate(FC.PAIRS):
        assert np.degrees(rotation_error(c.rotation(fa, fb), rot[p])) < 0.05
    be.close()


def test_the_python_mirror_returns_what_the_pose_stage_takes():
    c = FC.case("cut-200x168")
    be = backend_for(c.cam)
    s = c.statement
    got = SY.optical_flow_pyrlk(c.frames, FC.PAIRS, c.features, backend=be, width=c.width)
    for p, r in enumerate(got):
        assert np.array_equal(r[0], s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]]) and np.array_equal(r[1], s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]])
    got = SY.optical_flow_pyrlk(c.frames, [(0, 1)], [f[20:29] for f in c.features], backend=be, width=c.width)      # under 10 kept points: None (opencv_pyrlk.rs:107)
    assert got == [None]
    grid = SY.optical_flow_pyrlk(c.frames, FC.PAIRS, None, backend=be, width=c.width)
    g = c.grid_statement
    assert all(np.array_equal(r[1], g["points_b"][g["pair_first"][p]:g["pair_first"][p + 1]]) for p, r in enumerate(grid))
    be.close()
