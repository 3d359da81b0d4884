"""STMap 'undist' coordinate export (gfw_stmap_undistort) vs the oracle restatement of src/core/stmap.rs:87-109: lens models and shutters; the case table of
tests/_coordcase.py from a sentinel (rejected rays, the block edge, meshes, digital lenses, IBIS rows, one matrix); device outputs, synchronous and
asynchronous over the matrix staging ring; device-resident matrix tables; the context's rows limit; the map held to the render; the map fed to the point map."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
import _coordcase as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model,k", [("opencv_fisheye", [0.045, 0.02, -0.02, 0.006]), ("opencv_standard", [0.1, -0.05, 0.001, 0.002, 0.01, 0.0, 0.0, 0.0]),
                                     ("poly5", [0.08, -0.02]), ("sony", [1.0, 0.01, -0.05, 0.02, 0.0, 0.0]), ("gopro", [0.0, 1.0, 0.01, -0.12, 0.02, 0.01, -0.004])])
@pytest.mark.parametrize("hrs", [False, True])
def test_stmap_matches_oracle_bit_exact(model, k, hrs):
    w, h = 384, 216
    lens = S.gopro_style_lens(w, h)
    lens["model"] = model
    lens["k"] = list(k) + [0.0] * (12 - len(k))
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=5, lens=lens, horizontal_rs=hrs, fov=1.4)
    kp = fr.planes[0]["params"].copy()
    kp.flags = abi.FLAG_HORIZONTAL_RS if hrs else 0          # stmap.rs:36-38
    ref = O.stmap_undistort(kp, fr.model, 0, fr.matrices, w, h)
    pl = fr.planes[0]
    b = warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"])
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, 0, b)
    try:
        got = be.stmap_undistort(kp, fr.matrices, w, h)
    finally:
        be.close()
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    assert np.count_nonzero(ref) > 0.5 * ref.size


# ---- the case table of tests/_coordcase.py (the CPU tier runs the same inputs through the interpreter: tests/test_emu_coords.py) ----------------------------

def backend_for(fr):
    """A context with the frame's lens ids.  gfw_create refuses a plane of fewer than 4 rows (opencl.rs:179), so the 61 x 3 and 1 x 1 maps are asked of a context created
    for a 64 x 8 plane of the same lens: the map call brings its own KernelParams, the context the lens ids and the rows limit (8 >= their matrix counts)."""
    if fr.height < 4:
        assert not fr.planes[0]["params"].flags & abi.FLAG_HORIZONTAL_RS and fr.matrices.shape[0] <= 8
        fr = S.SyntheticFrame(fr.fmt, 64, 8, lens=fr.lens)
    pl = fr.planes[0]
    b = warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"])
    return warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, b)


def stmap_call(be, kp, matrices, matrix_count, mesh, w, h, out_ptr, on_device):
    """gfw_stmap_undistort as the C ABI has it -> its return code.  `matrices`: a host array, or a device pointer with `matrix_count`."""
    if isinstance(matrices, np.ndarray):
        assert matrices.dtype == np.float32 and matrices.flags.c_contiguous
        matrices, matrix_count = matrices.ctypes.data, matrices.shape[0]
    meshp, meshn = (mesh.ctypes.data, mesh.size) if mesh is not None else (None, 0)
    return be.lib.gfw_stmap_undistort(be.ctx, C.byref(kp), matrices, matrix_count, meshp, meshn, w, h, out_ptr, 1 if on_device else 0)


def sentinel_tensor(w, h, dev):
    """w * h * 2 + TAIL 32-bit elements on the device, every one the sentinel: the map and a tail nobody may touch"""
    import torch
    return torch.full((w * h * 2 + TAIL,), K.SENTINEL, dtype=torch.int32, device=dev)


def split(t, w, h):
    """-> (the map [h][w][2], the tail) of a sentinel_tensor as uint32"""
    u = t.cpu().numpy().view(np.uint32)
    return u[:w * h * 2].reshape(h, w, 2), u[w * h * 2:]


TAIL = 64


@pytest.mark.parametrize("name", K.NAMES)
def test_stmap_case_table_from_a_sentinel(name):
    """Host output through warp.Backend: the array goes up holding the sentinel, the kernel leaves rejected pixels alone, and what comes back is the oracle's
    map bit for bit (K.same_map: a NaN the arithmetic produced equals a produced NaN, the sentinel only itself) — r_limit, W <= 0, a saturating row pick, 203 x 117 and the shapes around one 64 x 4 workgroup, an f32 mesh (and with it the <-1>
    instantiation for a fisheye clip), the digital lenses, refraction, IBIS rows, one matrix."""
    fr, kp, mesh, w, h = K.case(name)
    ref = K.reference(name)
    be = backend_for(fr)
    try:
        got = be.stmap_undistort(kp, fr.matrices, w, h, mesh=mesh, fill=K.SENTINEL)
        assert warp.last_backend() == "stmap"
    finally:
        be.close()
    assert K.same_map(ref, got)


@pytest.mark.parametrize("name", ["rl_gopro", "mesh_fisheye", "block_65x5", "one"])
def test_stmap_into_device_memory(name):
    """coords_on_device = 1 on a synchronous context: the map is complete when the call returns, and the 64 elements behind it are intact."""
    import torch
    fr, kp, mesh, w, h = K.case(name)
    dev = torch.device("cuda", 0)
    out = sentinel_tensor(w, h, dev)
    torch.cuda.synchronize(dev)                              # (filled on torch's stream, written on the context's)
    be = backend_for(fr)
    try:
        assert stmap_call(be, kp, fr.matrices, None, mesh, w, h, out.data_ptr(), True) == 0, be.lib.gfw_last_error()
        got, tail = split(out, w, h)                         # straight after the call, no synchronize in between
        assert warp.Backend.last_backend_of(be) == "stmap"
    finally:
        be.close()
    assert K.same_map(K.reference(name), got)
    assert np.all(tail == K.SENTINEL)


def mat_slots():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gyroflow_amd", "csrc", "gfw_api.hip")).read()
    return int(re.search(r"kMatSlots\s*=\s*(\d+)\s*;", src).group(1))


def test_stmap_asynchronous_calls_reuse_the_matrix_staging_ring():
    """GFW_OPT_SYNCHRONOUS 0, device outputs: kMatSlots + 1 calls back to back, each with another frame's HOST matrix table and its own output tensor, one
    synchronize at the end.  The last call takes the first call's staging slot again; every map must still be its own frame's."""
    import torch
    n = mat_slots() + 1
    assert n >= 2
    w, h = K.W, K.H
    frames = [K._frame(w, h, "opencv_fisheye", 1.2, 120 + j, timestamp_ms=1000.0 + 41.7 * j) for j in range(n)]
    kps = [K.stmap_params(fr) for fr in frames]
    refs = [O.stmap_undistort(kp, fr.model, 0, fr.matrices, w, h, fill=K.SENTINEL) for fr, kp in zip(frames, kps)]
    for j in range(1, n):
        assert not np.array_equal(refs[0], refs[j])          # the frames' tables do differ: a stale slot would show
    dev = torch.device("cuda", 0)
    outs = [sentinel_tensor(w, h, dev) for _ in range(n)]
    torch.cuda.synchronize(dev)
    be = backend_for(frames[0])
    try:
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        for fr, kp, out in zip(frames, kps, outs):
            assert stmap_call(be, kp, fr.matrices, None, None, w, h, out.data_ptr(), True) == 0, be.lib.gfw_last_error()
        be.synchronize()
        got = [split(o, w, h) for o in outs]
    finally:
        be.close()
    for j, ((m, tail), ref) in enumerate(zip(got, refs)):
        assert K.same_map(ref, m), "call %d" % j
        assert np.all(tail == K.SENTINEL), "call %d" % j


@pytest.mark.parametrize("name", ["ibis_rs", "ibis_hrs"])
@pytest.mark.parametrize("mode", [1, 2])
def test_stmap_with_device_resident_matrices(mode, name):
    """GFW_OPT_MATRICES_ON_DEVICE 2: packed rows[16] in HBM; 1: raw rows[14] through gfw_repack_matrices_kernel — the IBIS case, so that the cos / sin
    slots the repack fills (and the 1 / 0 of the rows without IBIS data) are read."""
    import torch
    fr, kp, mesh, w, h = K.case(name)
    dev = torch.device("cuda", 0)
    host = np.ascontiguousarray(fr.matrices) if mode == 1 else warp.pack_matrices(fr.matrices)
    d_mat = torch.from_numpy(host.copy()).to(dev)
    out = sentinel_tensor(w, h, dev)
    torch.cuda.synchronize(dev)
    be = backend_for(fr)
    try:
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, mode)
        assert stmap_call(be, kp, d_mat.data_ptr(), fr.matrices.shape[0], None, w, h, out.data_ptr(), True) == 0, be.lib.gfw_last_error()
        got, tail = split(out, w, h)
    finally:
        be.close()
    assert K.same_map(K.reference(name), got)
    assert np.all(tail == K.SENTINEL)


def test_stmap_rows_limit_of_the_context():
    """A context holds matrix tables of at most the rows of the plane it was created for (height; width under a horizontal shutter).  stmap.rs sizes its undist
    map larger than the source, so a caller meets this: a map with more rows than the context's plane is refused — GFW_ERR_BUFFER_SIZE_MISMATCH, the reference's
    "Buffer size mismatch matrices!" — with nothing written, and served by a context created at the map's size."""
    import torch
    small = K.case("single")[0]                              # a 203 x 117 plane
    w, h = 203, 131
    fr = K._frame(w, h, "opencv_fisheye", 1.2, 121)
    kp = K.stmap_params(fr)
    assert fr.matrices.shape[0] == h > small.height
    ref = O.stmap_undistort(kp, fr.model, 0, fr.matrices, w, h, fill=K.SENTINEL)
    dev = torch.device("cuda", 0)
    out = sentinel_tensor(w, h, dev)
    torch.cuda.synchronize(dev)
    host = K.filled((h, w, 2))
    be = backend_for(small)
    try:
        for ptr, on_device in ((out.data_ptr(), True), (host.ctypes.data, False)):
            assert stmap_call(be, kp, fr.matrices, None, None, w, h, ptr, on_device) == -8         # GFW_ERR_BUFFER_SIZE_MISMATCH
            assert abi.ERRORS[-8] == "BufferSizeMismatch" and b"Buffer size mismatch matrices!" in be.lib.gfw_last_error()
        be.synchronize()
        assert np.all(out.cpu().numpy().view(np.uint32) == K.SENTINEL) and np.all(host.view(np.uint32) == K.SENTINEL)
    finally:
        be.close()
    be = backend_for(fr)
    try:
        assert stmap_call(be, kp, fr.matrices, None, None, w, h, out.data_ptr(), True) == 0, be.lib.gfw_last_error()
        got, tail = split(out, w, h)
    finally:
        be.close()
    assert K.same_map(ref, got) and np.all(tail == K.SENTINEL)


def test_the_undist_map_is_where_the_render_samples_on_the_device():
    """tests/test_stmap_statement.py with libgfwarp's render and libgfwarp's map (first fisheye case): same bound — 1/64 px + 2 ULP(200), derived from the
    sampler — and same inside share.  The kernel restates the row pick apart from the render's; this ties the two."""
    fr, mesh = K.ramp_frame("fisheye_1.4_rs")
    w, h = K.STATEMENT_W, K.STATEMENT_H
    kp = K.stmap_params(fr)
    share_o = K.map_against_render(K.render_rg(fr, O.run_frame(fr)[0]), O.stmap_undistort(kp, fr.model, 0, fr.matrices, w, h, fill=K.SENTINEL), w, h)[0]
    assert share_o >= K.INSIDE_SHARE                         # the condition on the inputs, on the oracle's output
    rg = K.render_rg(fr, warp.run_frame(fr)[0])
    be = backend_for(fr)
    try:
        coords = be.stmap_undistort(kp, fr.matrices, w, h, fill=K.SENTINEL)
    finally:
        be.close()
    share, worst, bound = K.map_against_render(rg, coords, w, h)
    print("device: inside share %.3f, max |render.rg - map| %.6f px (bound %.6f)" % (share, worst, bound))
    assert share >= K.INSIDE_SHARE and worst <= bound, (share, worst, bound)


def test_undist_map_fed_to_the_point_map():
    """The chain a caller builds: the undist map of `single` (out-of-frame coordinates included) as the points of gfw_undistort_points, GFW_POINT_INDEX_SINGLE,
    against the oracle given the same points.  (How well the pair inverts each other is tests/test_oracle_points.py's subject.)"""
    from test_gpu_points import same_bits
    from test_oracle_points import points_params
    fr, kp, mesh, w, h = K.case("single")
    pts = np.ascontiguousarray(K.reference("single").reshape(-1, 2))
    assert np.mean((pts[:, 0] < 0) | (pts[:, 0] > w) | (pts[:, 1] < 0) | (pts[:, 1] > h)) > 0.01             # (0.018 on the oracle)
    pp = points_params(fr)
    ref = O.undistort_points(pp, fr.model, 0, fr.rotations, points=pts, index_mode=abi.POINT_INDEX_SINGLE)
    be = backend_for(fr)
    try:
        got_map = be.stmap_undistort(kp, fr.matrices, w, h, fill=K.SENTINEL)
        got = be.undistort_points(pp, fr.rotations, points=got_map.reshape(-1, 2), index_mode=abi.POINT_INDEX_SINGLE)
        assert warp.last_backend() == "points"
    finally:
        be.close()
    assert same_bits(ref, got)
