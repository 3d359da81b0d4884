"""gfw_zoom_fovs_stab on the MI355X: the zoom search of clips with IBIS/OIS splines and per-frame lens meshes in one device call, against the host statement
(tests/_zoomstab.py) and the host-interpreted kernel under the rules of tests/test_emu_zoom_stab.py — bit-identical wherever no track is read, twice the measured
sensitivity (tests/golden/zoom_stab_sensitivity.json) with rotations from the tracks — and against the route it replaces: per frame and round one
gfw_undistort_points call with host-packed shifts and that frame's mesh (two where the frame has no rolling shutter: point 0 with the frame's one shift, the other
points with none — a call's shifts cannot say "none" for a single point), then the fold on the host."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _zoomstmt as Z
import _zoomstab as ZS
from test_gpu_zoom import backend_for, same_f64

pytestmark = pytest.mark.gpu

CLIPS = {c.name: c for c in ZS.stab_clips()}
SENS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoom_stab_sensitivity.json")))["clips"]


def device_fovs(clip, given_rotations=False, be=None, **kw):
    own = be is None
    be = be or backend_for(clip)
    try:
        kp, search, frames, rot, stabs, meshes = ZS.inputs(clip, given_rotations)
        if not given_rotations:
            be.set_quaternion_tracks(*clip.tracks)
            if clip.sync_offsets is not None:
                be.set_sync_offsets(clip.duration_ms, *clip.sync_offsets)
        out = be.zoom_fovs_stab(kp, search, frames, rotations=rot, stabs=stabs, meshes=meshes, debug=True, **kw)
        assert warp.last_backend() == "zoom_fovs_stab"
        return out
    finally:
        if own:
            be.close()


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_given_rotations_bit_identical_to_statement_and_emulator(name):
    clip = CLIPS[name].with_mode(0, readout=0.0)
    fov, dbg = device_fovs(clip, True)
    ref_f, ref_d = ZS.clip_fovs(clip, given_rotations=True)
    emu_f, emu_d = ZS.emu_clip_fovs(clip, given_rotations=True)
    assert same_f64(fov, ref_f), (name, fov, ref_f)
    assert same_f64(dbg, ref_d), name
    assert same_f64(fov, emu_f) and same_f64(dbg, emu_d), name


@pytest.mark.parametrize("mode,horizontal", [(1, False), (1, True), (2, False), (2, True)])
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_suppressed_rotation_with_rolling_shutter_bit_identical(name, mode, horizontal):
    clip = CLIPS[name].with_mode(mode, readout=12.0, horizontal=horizontal)
    fov, dbg = device_fovs(clip)
    ref_f, ref_d = ZS.clip_fovs(clip)
    assert same_f64(fov, ref_f), (name, mode, horizontal, fov, ref_f)
    assert same_f64(dbg, ref_d), (name, mode, horizontal)


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_rotations_from_tracks_within_the_measured_sensitivity(name):
    clip = CLIPS[name]
    fov, dbg = device_fovs(clip)
    ref_f, ref_d = ZS.clip_fovs(clip)
    rel, poly = float(np.max(np.abs(fov - ref_f) / ref_f)), float(np.max(np.abs(dbg - ref_d)))
    bar_f, bar_p = 2.0 * SENS[name]["fov_max_rel"], 2.0 * SENS[name]["polygon_max_abs"]
    print("%s: fov_minimal relative difference %.3g (bar %.3g), polygon %.3g (bar %.3g), %d of %d frames bit-identical"
          % (name, rel, bar_f, poly, bar_p, int(np.sum(fov == ref_f)), len(fov)))
    assert rel <= bar_f, (name, rel, bar_f)
    assert poly <= bar_p, (name, poly, bar_p)


@pytest.mark.parametrize("name,mode,readout", [("all-r0-poly5", 0, 0.0), ("all-r12-sony", 1, 12.0), ("shifts-r12-l0.6", 1, 12.0), ("all-r12-digital", 0, 0.0)])
def test_equals_the_route_it_replaces_over_a_few_hundred_frames(name, mode, readout):
    """240 frames (the clip's 24, ten times).  No track is read on either side: caller-given rotations without rolling shutter, suppress_rotation 1 with it."""
    clip = CLIPS[name].with_mode(mode, readout=readout)
    given = readout == 0.0
    tile = 10
    be = backend_for(clip)
    try:
        kp, search, frames, rot, stabs, meshes = ZS.inputs(clip, given, tile=tile)
        if not given:
            be.set_quaternion_tracks(*clip.tracks)                               # (required by the call; suppress_rotation 1 reads none of it)
        fov, dbg = be.zoom_fovs_stab(kp, search, frames, rotations=rot, stabs=stabs, meshes=meshes, debug=True)
        calls = [0]

        def points_fn(kpk, rotations, points, shifts, mesh):
            calls[0] += 1
            return be.undistort_points(kpk, rotations, points=points, shifts=shifts, index_mode=abi.POINT_INDEX_PER_POINT, mesh=mesh)
        old_f, old_d = [], []
        for k in range(24):
            f, d = ZS.frame_fov(clip, k, Z.frame_rotation(clip, k) if given else None, points_fn=points_fn)
            old_f.append(f)
            old_d.append(d)
        assert warp.last_backend() == "points" and calls[0] >= 48
    finally:
        be.close()
    assert same_f64(fov, np.tile(old_f, tile)), name
    assert same_f64(dbg, np.tile(np.array(old_d), (tile, 1, 1))), name


def test_null_tables_equal_gfw_zoom_fovs():
    clip = CLIPS["shifts-r12"]
    be = backend_for(clip)
    try:
        be.set_quaternion_tracks(*clip.tracks)
        kp, search, frames, _, stabs, _ = ZS.inputs(clip)
        for f in frames:
            f.suppress_rotation = 0
        a = be.zoom_fovs(kp, search, frames, debug=True)
        b = be.zoom_fovs_stab(kp, search, frames, debug=True)
        assert warp.last_backend() == "zoom_fovs"
        flagged = kp.copy()
        flagged.flags |= abi.FLAG_HAS_IBIS_DATA | abi.FLAG_HAS_MESH_DATA | abi.FLAG_HAS_FPD_DATA      # accepted, not consulted: the data decides
        c = be.zoom_fovs_stab(flagged, search, frames, debug=True)
        d = be.zoom_fovs_stab(kp, search, frames, stabs=[None] * 24, meshes=[None] * 24, debug=True)   # every entry absent: the other kernel, the same bits
        assert warp.last_backend() == "zoom_fovs_stab"
        e = be.zoom_fovs_stab(kp, search, frames, stabs=stabs, debug=True)
    finally:
        be.close()
    for other in (b, c, d):
        assert same_f64(a[0], other[0]) and same_f64(a[1], other[1])
    assert not same_f64(a[0], e[0])


def test_device_outputs_on_an_asynchronous_context_and_empty_clip():
    import torch
    dev = torch.device("cuda", 0)
    clip = CLIPS["all-r12-sony"].with_mode(1)
    ref_f, ref_d = ZS.clip_fovs(clip)
    tile = 50
    n = 24 * tile
    be = backend_for(clip)
    try:
        be.set_quaternion_tracks(*clip.tracks)
        kp, search, frames, _, stabs, meshes = ZS.inputs(clip, tile=tile)
        d_f = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        d_d = torch.full((n, 120, 2), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        assert be.zoom_fovs_stab(kp, search, frames, stabs=stabs, meshes=meshes, out_ptr=d_f.data_ptr(), debug_ptr=d_d.data_ptr()) is None
        first = (abi.ZoomFrame * 24).from_buffer(frames)
        be.zoom_fovs_stab(kp, search, first, stabs=stabs[:24], meshes=meshes[:24], out_ptr=d_f.data_ptr())          # a second call behind it, other tables in the same staging block
        be.synchronize()
        assert same_f64(d_f.cpu().numpy(), np.tile(ref_f, tile)) and same_f64(d_d.cpu().numpy(), np.tile(ref_d, (tile, 1, 1)))
        d_f.fill_(-3.0)
        torch.cuda.synchronize(dev)
        lib = be.lib
        st, keep = warp.frame_stab_table(stabs)
        assert lib.gfw_zoom_fovs_stab(be.ctx, C.byref(kp), C.byref(search), C.cast(frames, C.c_void_p), 0, None, st, None, None, d_f.data_ptr(), None, 1) == 0      # n_frames = 0
        assert lib.gfw_zoom_fovs_stab(be.ctx, C.byref(kp), C.byref(search), None, 0, None, None, None, None, None, None, 0) == 0
        be.synchronize()
        assert bool((d_f == -3.0).all())
    finally:
        be.close()
    torch.cuda.synchronize()


def small_backend(clip):
    """a context for the smallest plane gfw_create takes, 64 x 8, with the clip's lens ids: the zoom search brings its own KernelParams"""
    fr = S.SyntheticFrame("NV12", 64, 8, seed=3, lens=clip.lens, pixels=True)
    pl = fr.planes[0]
    return warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))


def test_the_staging_block_regrows_between_asynchronous_calls():
    """Three calls back to back on an asynchronous context, 2, 24 and 5 frames of a clip with stabiliser data and meshes, each into its own device tensors: the
    second call grows both sides of the one staging block while the first search may still read it, the third takes it smaller.  After one synchronize every
    result is the same call's on a synchronous context, bit for bit."""
    import torch
    dev = torch.device("cuda", 0)
    clip = CLIPS["all-r12-sony"].with_mode(1)
    kp, search, frames, _, stabs, meshes = ZS.inputs(clip)
    counts = (2, 24, 5)

    def call(be, k, **kw):
        return be.zoom_fovs_stab(kp, search, (abi.ZoomFrame * k).from_buffer(frames), stabs=stabs[:k], meshes=meshes[:k], **kw)
    be = small_backend(clip)
    try:
        be.set_quaternion_tracks(*clip.tracks)
        refs = [call(be, k, debug=True) for k in counts]
    finally:
        be.close()
    assert not same_f64(refs[0][0], refs[1][0][3:5])                                 # frames differ: another call's block would show
    d_f = [torch.full((k,), -1.0, dtype=torch.float64, device=dev) for k in counts]
    d_d = [torch.full((k, 120, 2), -1.0, dtype=torch.float64, device=dev) for k in counts]
    torch.cuda.synchronize(dev)
    be = small_backend(clip)
    try:
        be.set_quaternion_tracks(*clip.tracks)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        for k, f, d in zip(counts, d_f, d_d):
            assert call(be, k, out_ptr=f.data_ptr(), debug_ptr=d.data_ptr()) is None
        be.synchronize()
        got = [(f.cpu().numpy(), d.cpu().numpy()) for f, d in zip(d_f, d_d)]
    finally:
        be.close()
    for k, (f, d), (rf, rd) in zip(counts, got, refs):
        assert same_f64(f, rf) and same_f64(d, rd), k


def test_a_context_closed_with_work_enqueued_completes_it():
    """gfw_destroy drains both of the context's streams before anything is released: an asynchronous context takes one coordinate map into the caller's tensor
    (the matrix ring, copied on the auxiliary stream), one table build with stabiliser data into the caller's table and one zoom search into the caller's tensor,
    and is closed without a synchronize.  The three outputs are those of a synchronous context; a context created afterwards repeats a call correctly."""
    import torch
    import _coordcase as K
    from test_gpu_matrix_builder import _stab
    from test_gpu_stmap import sentinel_tensor, split, stmap_call
    dev = torch.device("cuda", 0)
    clip = CLIPS["shifts-r12"]
    assert clip.lens["model"] == "opencv_fisheye"
    w, h, n = 64, 8, 5
    fr = K._frame(w, h, "opencv_fisheye", 1.2, 120)
    skp = K.stmap_params(fr)
    nk = S.new_k(fr.lens, 1.0, w, h)
    kp, search, frames, _, stabs, _ = ZS.inputs(clip)
    frames = (abi.ZoomFrame * n).from_buffer(frames)

    def run(asynchronous, only_build=False):
        coords, table = sentinel_tensor(w, h, dev), torch.zeros((h, 16), dtype=torch.float32, device=dev)
        d_f = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        be = small_backend(clip)
        try:
            be.set_quaternion_tracks(*clip.tracks)
            be.set_option(abi.OPT_SYNCHRONOUS, 0 if asynchronous else 1)
            if not only_build:
                assert stmap_call(be, skp, fr.matrices, None, None, w, h, coords.data_ptr(), True) == 0, be.lib.gfw_last_error()
            be.build_matrices(nk, 1000.3, 16.0, h, h, stab=_stab(w, h), out_ptr=table.data_ptr())
            if not only_build:
                be.zoom_fovs_stab(kp, search, frames, stabs=stabs[:n], out_ptr=d_f.data_ptr())
        finally:
            be.close()                                       # no synchronize before it
        torch.cuda.synchronize(dev)
        return split(coords, w, h), table.cpu().numpy().view(np.uint32), d_f.cpu().numpy()
    (ref_map, ref_tail), ref_table, ref_f = run(False)
    assert np.any(ref_map != K.SENTINEL) and np.all(ref_tail == K.SENTINEL) and np.abs(ref_table.view(np.float32)[:, 9:14]).max() > 0.01 and np.all(ref_f > 0.0)
    (got_map, got_tail), got_table, got_f = run(True)
    assert np.array_equal(got_map, ref_map) and np.array_equal(got_tail, ref_tail)
    assert np.array_equal(got_table, ref_table)
    assert same_f64(got_f, ref_f)
    assert np.array_equal(run(False, only_build=True)[1], ref_table)


def test_arguments():
    import copy
    clip = CLIPS["all-r0-poly5"].with_mode(0, readout=0.0)
    kp, search, frames, rot, stabs, meshes = ZS.inputs(clip, True)
    be = backend_for(clip)
    lib, f = be.lib, be.lib.gfw_zoom_fovs_stab
    out = np.full(24, -7.0)
    fp, rp, op = C.cast(frames, C.c_void_p), rot.ctypes.data, out.ctypes.data
    INV = abi.ERR_INVALID_ARGUMENT

    def call(stabs_=stabs, meshes_=meshes, lens=None, rp_=rp, op_=op, fp_=fp, ctx=be.ctx):
        st, keep = warp.frame_stab_table(stabs_) if stabs_ is not None else (None, None)
        mp = lp = None
        if meshes_ is not None:
            mp, lp = (C.c_void_p * 24)(), (C.c_size_t * 24)()
            held = [None if m is None else np.ascontiguousarray(m, dtype=np.float64) for m in meshes_]
            for k, m in enumerate(held):
                if m is not None:
                    mp[k], lp[k] = m.ctypes.data, m.size
            if isinstance(lens, dict):
                for k, v in lens.items():
                    lp[k] = v
        return f(ctx, C.byref(kp), C.byref(search), fp_, 24, rp_, st, mp, None if lens == "null" else lp, op_, None, 0), lib.gfw_last_error()

    def broken(k, **changes):
        s = [None if st is None else dict(st) for st in stabs]
        s[k].update(changes)
        return s
    try:
        # a null required pointer
        assert call(ctx=None)[0] == INV and call(fp_=None)[0] == INV and call(op_=None)[0] == INV
        rc, msg = call(lens="null")
        assert rc == INV and b"mesh_lens" in msg
        ibis = np.asarray(stabs[6]["ibis"], dtype=np.float64)
        st, keep = warp.frame_stab_table(stabs)
        keep_ptr = C.cast(C.c_void_p(st[6]), C.POINTER(abi.FrameStab)).contents
        saved, keep_ptr.ibis = keep_ptr.ibis, None                                    # a count without its array
        assert f(be.ctx, C.byref(kp), C.byref(search), fp, 24, rp, st, None, None, op, None, 0) == INV and b"frame 6" in lib.gfw_last_error()
        keep_ptr.ibis = saved
        # descending spline positions
        down = ibis.copy()
        down[9, 0] = down[7, 0]
        rc, msg = call(stabs_=broken(6, ibis=down))
        assert rc == INV and b"frame 6" in msg and b"ascend" in msg
        od = np.asarray(stabs[9]["ois"], dtype=np.float64).copy()
        od[3, 0] = od[1, 0]
        rc, msg = call(stabs_=broken(9, ois=od))
        assert rc == INV and b"frame 9" in msg and b"ascend" in msg
        # zero crop or pitch
        rc, msg = call(stabs_=broken(3, crop_area=(120.0, 338.0, 0.0, 2700.0)))
        assert rc == INV and b"frame 3" in msg
        rc, msg = call(stabs_=broken(10, pixel_pitch=(3.0, 0.0)))
        assert rc == INV and b"frame 10" in msg
        # an oversized or inconsistent mesh
        big = list(meshes)
        big[13] = np.concatenate([meshes[13], np.zeros(1)])
        rc, msg = call(meshes_=big)
        assert rc == INV and b"frame 13" in msg and b"large" in msg
        bad = list(meshes)
        bad[5] = meshes[5].copy()
        bad[5][1] = 12.0                                                              # a 12 x 9 grid does not fit the block
        rc, msg = call(meshes_=bad)
        assert rc == INV and b"frame 5" in msg
        rc, msg = call(lens={14: 400})                                                # shorter than its own header says
        assert rc == INV and b"frame 14" in msg
        # a readout time with caller-given rotations; suppress_rotation 3
        frames[3].frame_readout_time_ms = 8.0
        rc, msg = call()
        assert rc == INV and b"frame 3" in msg
        frames[3].frame_readout_time_ms = 0.0
        frames[7].suppress_rotation = 3
        rc, msg = call()
        assert rc == INV and b"frame 7" in msg and b"suppress_rotation" in msg
        frames[7].suppress_rotation = 2
        assert call(rp_=None)[0] == INV and b"tracks" in lib.gfw_last_error()        # no tracks, no rotations
        assert np.all(out == -7.0)                                                    # nothing was written
        assert call()[0] == 0 and np.all(out > 0.0)                                   # suppress_rotation 2 is a value here
    finally:
        be.close()
