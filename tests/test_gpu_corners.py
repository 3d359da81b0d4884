"""gfw_corners_shi_tomasi on the MI355X: Shi-Tomasi corner detection of all frames in one device call, against the statement (tests/_cornerstmt.py).  Every sum is
an integer, every f32 operation is one rounding on both sides and the pick is a maximum over unique keys, so every comparison is bit for bit: no tolerance.  The
shapes and parameter variants are the interpreter tier's (tests/_cornercase.py; the statement's results shared with tests/test_emu_corners.py)."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, warp
import _cornercase as CC
import _flowcase as FC
import _posecase as PC
import _posestmt as PS
from test_gpu_flow import backend_for

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def be():
    b = backend_for(FC.case("cut-200x168").cam)
    yield b
    b.close()


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_device_equals_the_statement_to_the_bit(be, name):
    c = CC.case(name)
    for v in CC.VARIANTS:
        got = be.corners_shi_tomasi(c.frames, c.width, scores=True, **v)
        assert warp.last_backend() == "corners_shi_tomasi"
        CC.assert_equal_to_statement(got, CC.statement(name, **v), "%s %r" % (name, v))
    full = CC.statement(name)
    for m in (64, 8):                                                                # the cap is an exact prefix
        got = be.corners_shi_tomasi(c.frames, c.width, max_corners=m, scores=True)
        assert np.array_equal(got["counts"], np.minimum(full["counts"], m)) and np.array_equal(got["corners"], full["corners"][:, :m])


def test_without_the_optional_outputs_and_a_frame_alone(be):
    c = CC.case("cut-200x168")
    want = CC.statement("cut-200x168")
    got = be.corners_shi_tomasi(c.frames, c.width, packed=False)
    assert sorted(got) == ["corners", "counts"]
    CC.assert_equal_to_statement(got, want, "no optional outputs", ("corners", "counts"))
    got = be.corners_shi_tomasi(c.frames[1:2], c.width)
    assert np.array_equal(got["corners"][0], want["corners"][1]) and got["feat_first"].tolist() == [0, 179]
    got = be.corners_shi_tomasi(np.zeros((0, 168, 208), dtype=np.uint8), 200)       # n_frames = 0 succeeds and writes nothing
    assert got["corners"].shape == (0, 200, 2) and got["feat_first"].tolist() == [0] and got["features"].shape == (0, 2)


def test_batches_equal_one_batch(be):
    """tests/test_emu_corners.py says why: 1 MiB holds the list of one 384 x 216 frame (three batches), 2 MiB of three (five frames: 3 + 2)"""
    c = CC.case("odd-384x216")
    want = CC.statement("odd-384x216")
    CC.assert_equal_to_statement(be.corners_shi_tomasi(c.frames, c.width, scores=True, max_workspace_mb=1), want, "three batches")
    order = [0, 1, 2, 0, 1]
    got = be.corners_shi_tomasi(c.frames[order], c.width, scores=True, max_workspace_mb=2)
    for name in ("corners", "scores", "counts"):
        assert np.array_equal(got[name].view(np.uint32), want[name][order].view(np.uint32)), name
    assert np.array_equal(got["features"], np.concatenate([want["corners"][f, :want["counts"][f]] for f in order]))


ORDER = ("corners", "scores", "counts", "feat_first", "features")


def device_outputs(n, m=200):
    import torch
    dev = torch.device("cuda", 0)
    full = lambda shape, v, t: torch.full(shape, v, dtype=t, device=dev)
    return {"corners": full((n, m, 2), -7.0, torch.float32), "scores": full((n, m), -7.0, torch.float32), "counts": full((n,), -7, torch.int32),
            "feat_first": full((n + 1,), -7, torch.int32), "features": full((n * m, 2), -7.0, torch.float32)}


def fetch(outs):
    got = {k: outs[k].cpu().numpy() for k in ORDER}
    kept = int(got["feat_first"][-1])
    assert (got["features"][kept:] == -7.0).all()                                    # only the kept entries are written
    got["features"] = got["features"][:kept]
    return got


def test_device_frames_and_device_outputs_agree(be):
    import torch
    c = CC.case("cut-200x168")
    want = CC.statement("cut-200x168")
    d_frames = torch.from_numpy(c.frames.copy()).to(torch.device("cuda", 0))
    outs = device_outputs(3)
    torch.cuda.synchronize()
    be.corners_shi_tomasi(d_frames.data_ptr(), c.width, out_ptrs=tuple(outs[k].data_ptr() for k in ORDER), shape=c.frames.shape)
    CC.assert_equal_to_statement(fetch(outs), want, "device frames and outputs")
    # device frames and outputs without the optional arrays
    outs = device_outputs(3)
    torch.cuda.synchronize()
    be.corners_shi_tomasi(d_frames.data_ptr(), c.width, out_ptrs=(outs["corners"].data_ptr(), None, outs["counts"].data_ptr(), None, None), shape=c.frames.shape)
    got = {k: outs[k].cpu().numpy() for k in ORDER}
    CC.assert_equal_to_statement(got, want, "device outputs, no optional arrays", ("corners", "counts"))
    assert (got["scores"] == -7.0).all() and (got["feat_first"] == -7).all() and (got["features"] == -7.0).all()
    # device frames, host outputs; host frames, device outputs
    CC.assert_equal_to_statement(be.corners_shi_tomasi(d_frames.data_ptr(), c.width, scores=True, shape=c.frames.shape), want, "device frames")
    outs = device_outputs(3)
    torch.cuda.synchronize()
    be.corners_shi_tomasi(c.frames, c.width, out_ptrs=tuple(outs[k].data_ptr() for k in ORDER))
    CC.assert_equal_to_statement(fetch(outs), want, "host frames, device outputs")


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots, other data each time, queued without waiting"""
    import torch
    dev = torch.device("cuda", 0)
    calls = [("cut-200x168", {}), ("odd-384x216", dict(max_workspace_mb=1)), ("noise-40x48", {})]
    assert len(calls) == abi.CORNERS_RING_SLOTS + 1
    b = backend_for(FC.case("cut-200x168").cam)
    outs = [device_outputs(len(CC.case(name).frames)) for name, _ in calls]
    torch.cuda.synchronize(dev)
    b.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    b.set_option(abi.OPT_SYNCHRONOUS, 0)
    for (name, kw), o in zip(calls, outs):
        c = CC.case(name)
        b.corners_shi_tomasi(c.frames, c.width, out_ptrs=tuple(o[k].data_ptr() for k in ORDER), **kw)
    b.synchronize()
    for (name, _), o in zip(calls, outs):
        CC.assert_equal_to_statement(fetch(o), CC.statement(name), name + " queued")
    b.close()


def test_every_rejection_gives_the_reason_and_leaves_the_outputs_untouched(be):
    c = CC.case("cut-200x168")
    outs = [np.full((3, 200, 2), -7.0, dtype=np.float32), np.full((3, 200), -7.0, dtype=np.float32), np.full(3, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32),
            np.full((600, 2), -7.0, dtype=np.float32)]
    p = lambda a: None if a is None else a.ctypes.data
    base = dict(width=c.width, height=c.height, stride=c.stride, max_corners=200, quality=0.01, min_distance=10.0)

    def call(cfg=None, frames=c.frames, n_frames=3, outs_=None):
        cfg = abi.CornersCfg(**dict(base, **(cfg or {})))
        return be.lib.gfw_corners_shi_tomasi(be.ctx, C.byref(cfg), p(frames), 0, n_frames, *[p(o) for o in (outs_ or outs)], 0)

    def refused(text, **kw):
        rc = call(**kw)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert all((o == -7).all() for o in outs)

    assert call() == 0                                                               # the arguments as they are succeed ..
    kept = int(outs[3][-1])
    CC.assert_equal_to_statement(dict(zip(ORDER, outs[:4] + [outs[4][:kept]])), CC.statement("cut-200x168"), "raw call")
    assert (outs[4][kept:] == -7.0).all()
    for o in outs:
        o[...] = -7                                                                  # .. and every variation below is refused
    refused("negative count", n_frames=-1)
    refused("4097 frames", n_frames=abi.CORNERS_FRAMES_MAX + 1)
    refused("3 frames without their planes", frames=None)
    refused("null corners / counts", outs_=[None] + outs[1:])
    refused("null corners / counts", outs_=outs[:2] + [None] + outs[3:])
    refused("both or neither", outs_=outs[:3] + [None, outs[4]])
    refused("both or neither", outs_=outs[:4] + [None])
    refused("frames of 2 x 168", cfg=dict(width=2))
    refused("frames of 200 x 8193", cfg=dict(height=8193))
    refused("stride 199 under the width 200", cfg=dict(stride=199))
    refused("max_corners 0", cfg=dict(max_corners=0))
    refused("max_corners 4097", cfg=dict(max_corners=4097))
    refused("quality 0,", cfg=dict(quality=0.0))
    refused("quality 1.5", cfg=dict(quality=1.5))
    refused("quality nan", cfg=dict(quality=float("nan")))
    refused("min_distance -1", cfg=dict(min_distance=-1.0))
    refused("min_distance 1025", cfg=dict(min_distance=1025.0))
    refused("min_distance inf", cfg=dict(min_distance=float("inf")))
    refused("max_workspace_mb -1 is negative", cfg=dict(max_workspace_mb=-1))
    refused("reserved", cfg=dict(reserved=1))
    refused("at most 2 GiB", cfg=dict(stride=1 << 20, height=8192))                  # 3 host frames of 8 GiB each: refused unread
    refused("is too small: the candidate list of ONE 2000 x 168 frame needs 2653344 bytes (3 MB)", cfg=dict(width=2000, stride=2000, max_workspace_mb=2))


def test_frames_to_rotations_through_the_three_device_calls(be):
    """frames -> gfw_corners_shi_tomasi -> gfw_flow_pyrlk -> gfw_pose_almeida (the packed arrays copied back between the calls: the next stages take theirs from
    host memory) equals the CPU chain (the three statements) to the bit on cut-200x168"""
    name = "cut-200x168"
    c, fc = CC.case(name), FC.case(name)
    cam = fc.cam
    feats = SY.detect_features_pyrlk(c.frames, be, width=c.width)
    want = CC.statement(name)
    for f in range(3):
        assert np.array_equal(feats[f], want["corners"][f, :want["counts"][f]])
    pairs = SY.optical_flow_pyrlk(c.frames, FC.PAIRS, feats, backend=be, width=c.width)
    want_pairs = CC.chain_pairs(name)
    assert all(p is not None and np.array_equal(p[0], w[0]) and np.array_equal(p[1].view(np.uint32), w[1].view(np.uint32)) for p, w in zip(pairs, want_pairs))
    triples, _ = PC.draws([len(a) for a, _ in want_pairs], cam.num_iters, cam.num_samples, 77, False)
    got = be.pose_almeida(cam.kp, PC.cfg_of(cam), pairs, triples)
    assert warp.last_backend() == "pose_almeida"
    PC.assert_equal_to_statement(got, PS.estimate(cam, want_pairs, triples, None)[:3], "frames to rotations")
