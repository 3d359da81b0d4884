"""gfw_flow_dis_refined on the MI355X: the DIS dense flow with its variational refinement on every level, all frame pairs in one device call, against the statement
(tests/_varrefstmt.py).  Every f32 operation is one rounding on both sides and every sum has one order, so every comparison is bit for bit: no tolerance.  The
shapes are the interpreter tier's (tests/_discase.CONFIGS: the three scenes at both finest scales — refined levels of 24 x 16 up to 96 x 54 at the reference's
finest scale 2, up to 192 x 108 at 1: odd widths, sizes that are no multiple of a workgroup's 256 lanes, several workgroups a pair); the statement's results are
shared with tests/test_emu_varref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, warp
import _discase as DC
import _varrefcase as VC
from test_cpp_dis import LIBDIR, ROOT, pair_lines
from test_gpu_dis import ORDER, backend_for, device_outputs, fetch

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name,finest", DC.CONFIGS)
def test_the_device_equals_the_statement_to_the_bit_from_host_and_device_memory(name, finest):
    """all four combinations: host and device frames x host and device outputs; with device outputs only the returned entries are written (fetch)"""
    import torch
    c = DC.case(name)
    want = VC.statement(name, finest)
    be = backend_for(c.cam)
    d_frames = torch.from_numpy(c.frames).to(torch.device("cuda", 0))
    DC.assert_equal_to_statement(be.flow_dis(c.frames, c.width, c.pairs, finest, flow=True, variational_iters=5), want, "%s finest %d: host frames, host outputs" % (name, finest))
    assert warp.last_backend() == "flow_dis_refined"
    DC.assert_equal_to_statement(be.flow_dis(d_frames.data_ptr(), c.width, c.pairs, finest, flow=True, shape=c.frames.shape, variational_iters=5), want, name + ": device frames, host outputs")
    for frames, shape, what in ((c.frames, None, "host frames"), (d_frames.data_ptr(), c.frames.shape, "device frames")):
        outs = device_outputs(c, len(c.pairs), finest)
        torch.cuda.synchronize()
        nodes = warp.flow_grid_nodes(c.width, c.height)
        assert be.flow_dis(frames, c.width, c.pairs, finest, out_ptrs=tuple(outs[k].data_ptr() for k in ORDER), shape=shape, variational_iters=5) == len(c.pairs) * nodes
        DC.assert_equal_to_statement(fetch(outs), want, "%s: %s, device outputs" % (name, what))
    be.close()


def test_another_configuration_no_iteration_a_pair_alone_and_no_pairs():
    c = DC.case("cut-200x168")
    be = backend_for(c.cam)
    o = VC.OTHER
    ref = abi.varref_cfg(sor_iters=o.sor_iters, alpha=o.alpha, delta=o.delta, gamma=o.gamma, omega=o.omega)
    got = be.flow_dis(c.frames, c.width, c.pairs, flow=True, variational_iters=o.fixed_point_iters, varref=ref)
    DC.assert_equal_to_statement(got, VC.statement("cut-200x168", 2, o), "2 fixed-point and 3 SOR iterations")
    # fixed_point_iters = 0 through the refined call: gfw_flow_dis to the bit
    plain = be.flow_dis(c.frames, c.width, c.pairs, flow=True)
    assert warp.last_backend() == "flow_dis"
    zero = be.flow_dis(c.frames, c.width, c.pairs, flow=True, variational_iters=0, varref=abi.varref_cfg())
    assert warp.last_backend() == "flow_dis_refined"
    for k in plain:
        assert np.array_equal(zero[k].view(np.uint32), plain[k].view(np.uint32)), k
    DC.assert_equal_to_statement(zero, DC.statement("cut-200x168", 2)[0], "fixed_point_iters = 0")
    # a pair equals its own single-pair call
    s = VC.statement("cut-200x168", 2)
    one = be.flow_dis(c.frames, c.width, [c.pairs[2]], flow=True, variational_iters=5)
    assert np.array_equal(one["points_b"].view(np.uint32), s["points_b"][s["pair_first"][2]:].view(np.uint32)) and np.array_equal(one["flow"][0].view(np.uint32), s["flow"][2].view(np.uint32))
    assert one["pair_first"].tolist() == [0, s["pair_first"][3] - s["pair_first"][2]]
    # no pairs succeed and write nothing
    got = be.flow_dis(c.frames, c.width, np.zeros((0, 2), dtype=np.int32), variational_iters=5)
    assert got["pair_first"].tolist() == [0] and got["points_a"].shape == (0, 2) and (got["grid_counts"] == 0).all()
    be.close()


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots():
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring (gfw_flow_dis's) has slots, other data each time, queued without waiting"""
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
        be.flow_dis(c.frames, c.width, c.pairs, finest, out_ptrs=tuple(o[k].data_ptr() for k in ORDER), variational_iters=5)
    be.synchronize()
    for (name, finest), o in zip(calls, outs):
        DC.assert_equal_to_statement(fetch(o), VC.statement(name, finest), name + " queued")
    be.close()


def test_every_rejection_names_its_reason_and_leaves_the_outputs_untouched():
    c = DC.case("cut-200x168")
    be = backend_for(c.cam)
    pf = np.ascontiguousarray(c.pairs, dtype=np.int32)
    nodes = warp.flow_grid_nodes(c.width, c.height)
    outs = [np.full((3, nodes, 2), -7.0, dtype=np.float32), np.full(3, -7, dtype=np.int32), np.full((3, 42, 50, 2), -7.0, dtype=np.float32),
            np.full(4, -7, dtype=np.int32), np.full((3 * nodes, 2), -7.0, dtype=np.float32), np.full((3 * nodes, 2), -7.0, dtype=np.float32)]
    p = lambda a: None if a is None else a.ctypes.data
    cfg = lambda **kw: abi.FlowDisCfg(**dict(dict(width=c.width, height=c.height, stride=c.stride, finest_scale=2), **kw))

    def call(cfg_=None, ref=None, frames=c.frames, n_frames=3, pf_=pf, n_pairs=3, outs_=None):
        cfg_, ref = cfg_ or cfg(), ref or abi.varref_cfg()
        return be.lib.gfw_flow_dis_refined(be.ctx, C.byref(cfg_), C.byref(ref), p(frames), 0, n_frames, p(pf_), n_pairs, *[p(o) for o in (outs_ or outs)], 0)

    def refused(text, **kw):
        rc = call(**kw)
        msg = be.lib.gfw_last_error().decode()
        assert rc == INV and text in msg, (rc, text, msg)
        assert all((o == -7).all() for o in outs)

    assert call() == 0                                                               # the arguments as they are succeed ..
    total = int(outs[3][-1])
    DC.assert_equal_to_statement(dict(zip(ORDER, outs[:4] + [outs[4][:total], outs[5][:total]])), VC.statement("cut-200x168", 2), "raw call")
    assert (outs[4][total:] == -7.0).all() and (outs[5][total:] == -7.0).all()
    for o in outs:
        o[...] = -7                                                                  # .. and every variation below is refused
    R = abi.varref_cfg
    refused("variational_iters 5 in gfw_flow_dis_cfg beside fixed_point_iters 5 in gfw_flow_varref_cfg", cfg_=cfg(variational_iters=5))
    refused("variational_iters 2 in gfw_flow_dis_cfg beside fixed_point_iters 0", cfg_=cfg(variational_iters=2), ref=R(fixed_point_iters=0))
    refused("fixed_point_iters -1 (0 to 64)", ref=R(fixed_point_iters=-1))
    refused("fixed_point_iters 65 (0 to 64)", ref=R(fixed_point_iters=65))
    refused("sor_iters 0 (1 to 64)", ref=R(sor_iters=0))
    refused("sor_iters 65 (1 to 64)", ref=R(sor_iters=65))
    for name in ("alpha", "delta", "gamma"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused("(finite and above 0)", ref=R(**{name: bad}))
            assert ("refinement configuration: %s " % name) in be.lib.gfw_last_error().decode()
    for bad in (0.0, 2.0, -0.5, float("nan"), float("inf")):
        refused("(between 0 and 2, both excluded)", ref=R(omega=bad))
    for k in (0, 1):
        ref = R()
        ref.reserved[k] = 1
        refused("refinement configuration: the reserved slots", ref=ref)
    # what gfw_flow_dis refuses is refused here in its words
    refused("negative count", n_pairs=-1)
    refused("without pair_frames", pf_=None)
    refused("3 frames without their planes", frames=None)
    refused("a null out_pair_first", outs_=outs[:3] + [None] + outs[4:])
    refused("pair 1: frames (1, 3) outside the call's 3 frames", pf_=np.array([[0, 1], [1, 3], [0, 2]], dtype=np.int32))
    refused("pair 2: frame 2 paired with itself", pf_=np.array([[0, 1], [1, 2], [2, 2]], dtype=np.int32))
    refused("frames of 256 x 24 have the coarsest scale 1, under the finest scale 2", cfg_=cfg(width=256, height=24, stride=256))
    refused("stride 199 under the width 200", cfg_=cfg(stride=199))
    refused("finest_scale 3", cfg_=cfg(finest_scale=3))
    refused("DIS flow configuration: the reserved slot", cfg_=cfg(reserved=1))
    refused("65536 pairs", n_pairs=abi.DIS_PAIRS_MAX + 1)
    rc = be.lib.gfw_flow_dis_refined(be.ctx, C.byref(cfg()), None, p(c.frames), 0, 3, p(pf), 3, *[p(o) for o in outs], 0)
    assert rc == INV and "null context / configuration" in be.lib.gfw_last_error().decode() and all((o == -7).all() for o in outs)
    be.close()


def test_the_python_mirror_returns_what_the_pose_stage_takes():
    c = DC.case("cut-200x168")
    be = backend_for(c.cam)
    for finest in DC.FINEST:
        s = VC.statement("cut-200x168", finest)
        got = SY.optical_flow_dis(c.frames, c.pairs, backend=be, width=c.width, finest_scale=finest, variational_iters=5)
        assert warp.last_backend() == "flow_dis_refined"
        for p, r in enumerate(got):
            assert np.array_equal(r[0], s["points_a"][s["pair_first"][p]:s["pair_first"][p + 1]]) and np.array_equal(r[1], s["points_b"][s["pair_first"][p]:s["pair_first"][p + 1]])
    be.close()


def test_the_cpp_mirror_equals_the_statement(tmp_path):
    """gyroflow::optical_flow_dis(.., finest_scale, 5) of include/gfwarp.hpp driven by tests/cpp/test_varref.cpp against a dump of the refined statement's points"""
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    exe = str(tmp_path / "test_varref")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_varref.cpp"), "-o", exe, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    name = "cut-200x168"
    c = DC.case(name)
    lines = [bytes(c.cam.kp).hex(), "%d %d" % (c.cam.clip.model, c.cam.clip.digital), "3 %d %d %d" % (c.width, c.height, c.stride), str(len(c.pairs))]
    lines += ["%d %d" % p for p in c.pairs]
    lines += pair_lines(VC.statement(name, 2)) + pair_lines(VC.statement(name, 1))
    path, frames = str(tmp_path / "varref.txt"), str(tmp_path / "frames.bin")
    open(path, "w").write("\n".join(lines) + "\n")
    c.frames.tofile(frames)
    r = subprocess.run([exe, "flow", path, frames], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "flow ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
