"""gfw_build_matrices_batch_stab on the MI355X: 64 frames of a clip with IBIS/OIS splines in one in-order launch — frames with and without stabiliser data,
both framebuffer orientations, suppress_rotation 0 / 1 / 2 (tests/_zoomstab.batch_case) — every table bit-identical to gfw_build_matrices_stab of the same frame;
and a gfw_undistort_clip_params launch fed those device tables bit-exact against the oracle fed the same rows."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
import _hoststmt as HS
import _zoomstab as ZS
from test_gpu_matrix_builder import fetch_rows, ulps
from test_gpu_parity import assert_plane_equal
from test_gpu_fullsize import _View

pytestmark = pytest.mark.gpu

W, H = 320, 192


def tracks():
    return S.sampled_track(21, 0.0, 3000.0, 1000.0), S.sampled_track(22, 0.0, 3000.0, 200.0, scale=0.25)


def build_batch(be, timings, stabs):
    n = len(timings)
    table, keep = warp.frame_stab_table(stabs)
    ptrs = (C.c_void_p * n)()
    be._check(be.lib.gfw_build_matrices_batch_stab(be.ctx, timings, table, n, ptrs))
    return [p for p in ptrs]


def test_sixty_four_tables_equal_the_single_frame_entry_bit_for_bit():
    fr = S.SyntheticFrame("YUV422P16LE", W, H, seed=9)
    org, sm = tracks()
    nk = S.new_k(fr.lens, 1.0, W, H)
    timings, stabs = ZS.batch_case(64, W, H, nk)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, 0, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    try:
        be.set_quaternion_tracks(org, sm)
        ptrs = build_batch(be, timings, stabs)
        assert len(set(ptrs)) == 64
        batch = [fetch_rows(p, H) for p in ptrs]
        again = build_batch(be, timings, stabs)                                  # the two context-owned batches alternate
        assert set(again).isdisjoint(ptrs) and build_batch(be, timings, stabs) == ptrs
        plain = be.build_matrices_batch(nk, [t.timestamp_ms for t in timings], 16.0, H, H, stabs=None)
        for k in range(64):
            t = timings[k]
            ptr = C.c_void_p(0)
            st = warp.frame_stab(stabs[k])[0] if stabs[k] is not None else None
            be._check(be.lib.gfw_build_matrices_stab(be.ctx, C.byref(t), C.byref(st) if st is not None else None, None, C.byref(ptr)))
            single = fetch_rows(ptr.value, H)
            assert np.array_equal(batch[k].view(np.uint32), single.view(np.uint32)), k
            has_terms = stabs[k] is not None and t.suppress_rotation != 2
            assert (np.abs(batch[k][:, 9:14]).max() > 0.05) == has_terms, k
        for k in (0, 3, 5, 9, 32):                                                   # ... and the f64 statement's bar on a few of them
            t = timings[k]
            host = HS.row_matrices_from_tracks(org, sm, nk, t.timestamp_ms, t.frame_readout_time_ms, H, H, framebuffer_inverted=bool(t.framebuffer_inverted),
                                               per_frame_offset_ms=t.per_frame_time_offset_ms, suppress_rotation=t.suppress_rotation, stab=stabs[k])
            scale = np.abs(host[:, :9]).max(axis=1, keepdims=True) * 1e-4
            assert ulps(batch[k][:, :9], host[:, :9], scale).max() <= 2.0, k
            assert ulps(batch[k][:, 9:14], host[:, 9:14], np.full((H, 1), 1e-6)).max() <= 1.0, k
        # the Python mirror takes the same tables
        mirror = be.build_matrices_batch(nk, [t.timestamp_ms for t in timings], 16.0, H, H, per_frame_offset_ms=0.0, stabs=stabs,
                                         framebuffer_inverted=[bool(t.framebuffer_inverted) for t in timings], suppress_rotation=[t.suppress_rotation for t in timings])
        zero_offset = [k for k in range(64) if timings[k].per_frame_time_offset_ms == 0.0]
        for k in zero_offset[:6]:
            assert np.array_equal(fetch_rows(mirror[k], H).view(np.uint32), batch[k].view(np.uint32)), k
        assert len(plain) == 64
        # a rejected frame is named
        bad = list(stabs)
        bad[12] = dict(stabs[12], crop_area=(120.0, 338.0, 5760.0, 0.0))
        with pytest.raises(warp.GfwError) as e:
            build_batch(be, timings, bad)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and "frame 12" in str(e.value)
        down = np.asarray(stabs[3]["ibis"], dtype=np.float64).copy()
        down[5, 0] = down[2, 0]
        bad = list(stabs)
        bad[3] = dict(stabs[3], ibis=down)
        with pytest.raises(warp.GfwError) as e:
            build_batch(be, timings, bad)
        assert "frame 3" in str(e.value) and "ascend" in str(e.value)
        with pytest.raises(warp.GfwError):
            build_batch(be, (abi.FrameTiming * 65)(), [None] * 65)
    finally:
        be.close()


def test_clip_params_launch_fed_the_batch_tables_is_bit_exact_against_the_oracle():
    import torch
    dev = torch.device("cuda", 0)
    n = 16
    frames = [S.SyntheticFrame("YUV422P16LE", W, H, seed=0x6A0 + f, timestamp_ms=1000.0 + 33.3 * f, fov=1.0 + 0.01 * f, pixels=False, flags=abi.FLAG_HAS_IBIS_DATA,
                               base_overrides={"translation2d": (-3.5 + 0.5 * f, 2.25 - 0.25 * f)}) for f in range(n)]
    org, sm = tracks()
    nk = S.new_k(frames[0].lens, 1.0, W, H)
    timings, stabs = ZS.batch_case(64, W, H, nk)
    d_src = [fr.device_planes(dev) for fr in frames]
    d_dst = [fr.device_outputs(dev) for fr in frames]
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [[pl["params"] for pl in fr.planes] for fr in frames]
    assert all(p.flags & abi.FLAG_HAS_IBIS_DATA and p.matrix_count == H for fp in params for p in fp)
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(), d_dst[j][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
    be = warp.Backend(params[0][0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    try:
        be.set_quaternion_tracks(org, sm)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        ptrs = build_batch(be, timings, stabs)                                   # asynchronous: the launch below follows it on the stream
        warp.ClipParamsCall(be, bufs, params, types, ptrs[:n], H)()
        be.synchronize()
        backend = warp.last_backend()
        rows = [fetch_rows(p, H) for p in ptrs[:n]]
    finally:
        be.close()
    torch.cuda.synchronize(dev)
    assert backend.startswith("yuv_fused"), backend
    assert sum(np.abs(r[:, 9:14]).max() > 0.05 for r in rows) >= 8
    for j, fr in enumerate(frames):
        fr.matrices = np.ascontiguousarray(rows[j][:, :14])
        srcs = [t.cpu().numpy() for t in d_src[j]]
        for p, (a, b) in enumerate(zip(O.run_frame(_View(fr, srcs)), [t.cpu().numpy() for t in d_dst[j]])):
            assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "clip_params over batch tables, frame %d plane %d" % (j, p))
