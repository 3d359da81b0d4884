"""The ONE context-owned buffer behind the host outputs of gfw_undistort_points, gfw_zoom_fovs*, gfw_sync_visual_* and gfw_sync_gyro_* (CallOutputs,
gyroflow_amd/csrc/gfw_hostmem.h; the STMap export uses it too and is not called here) on the MI355X: calls of different entry points, of different sizes (the buffer grows in the middle), one after the other on one
synchronous context — every result equals, to the bit, the same call on a fresh context.  Then the two searches on an asynchronous context with device outputs:
after synchronize() they equal the host-output results.  Both sides of a comparison run the same output helper: what this test sees is one call's results
left behind for, or overwritten by, another; that a call's own slices do not overlap is what the statement tests of each entry point see."""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _synccase as SC
import _syncgyrostmt as G
import _zoomcase as ZC
import _zoomstmt as Z

pytestmark = pytest.mark.gpu

CLIP = SC.CLIPS["fisheye-r0"]


def backend():
    fr = S.SyntheticFrame("NV12", CLIP.size[0], CLIP.size[1], seed=3, lens=CLIP.lens, pixels=True)
    pl = fr.planes[0]
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    be.set_quaternion_tracks(*CLIP.tracks)
    return be


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def calls():
    """[(name, call(backend) -> tuple of arrays)] in the order they share the buffer"""
    rng = np.random.default_rng(11)
    kp, search, frames, _ = ZC.inputs(CLIP, tile=2)
    f40, f3 = (abi.ZoomFrame * 40).from_buffer(frames), (abi.ZoomFrame * 3).from_buffer(frames)
    pkp, rot = CLIP.kernel_params(), np.asarray(Z.frame_rotation(CLIP, 0), dtype=np.float32).reshape(1, 9)
    pts = rng.uniform(0.0, 1.0, (16, 2)).astype(np.float32) * np.array(CLIP.size, dtype=np.float32)
    spts = lambda: rng.uniform(20.0, 160.0, (5, 2)).astype(np.float32)
    pairs = [(int(t * 1000.0), int((t + SC.GAP_MS) * 1000.0), spts(), spts()) for t in SC.TIMES[:2]]
    ssearch = SC.sync_search(CLIP)
    ranges = [G.make_range(40, 400, seed=3)]

    def points(be):
        return (be.undistort_points(pkp, rot, points=pts),)

    def visual(be):
        res, coarse, fine = be.sync_visual_search(kp, ssearch, pairs, 0, initial_offset_ms=5.0, search_size_ms=6.0, costs=True)
        return np.frombuffer(bytes(res), dtype=np.uint8), coarse, fine

    def gyro(be):
        res, coarse, fine = be.sync_gyro_search(ranges, 10.0, 8.0, costs=True)
        return np.frombuffer(b"".join(bytes(r) for r in res), dtype=np.uint8), coarse, fine

    return [("points", points), ("zoom of 40 with debug points", lambda be: be.zoom_fovs(kp, search, f40, debug=True)), ("visual search", visual), ("gyro search", gyro),
            ("zoom of 3", lambda be: (be.zoom_fovs(kp, search, f3),)), ("points again", points)], (kp, ssearch, pairs, ranges)


def test_calls_that_share_the_output_buffer_equal_the_same_calls_on_fresh_contexts(calls):
    import torch
    seq, (kp, ssearch, pairs, ranges) = calls
    shared, got = backend(), {}
    try:
        for name, call in seq:
            got[name] = call(shared)
            fresh = backend()
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got[name]) == len(want) and all(same_bits(a, b) for a, b in zip(got[name], want)), name
        assert got["zoom of 40 with debug points"][0].shape == (40,) and np.all(got["zoom of 40 with debug points"][0] > 0.0)
        assert got["visual search"][1].shape == (6,) and got["gyro search"][1].shape == (1, 16)
    finally:
        shared.close()
    # asynchronous, device outputs: nothing of the shared buffer is involved, the results are the same
    dev = torch.device("cuda", 0)
    be = backend()
    try:
        d = {k: torch.full((n,), -1.0, dtype=torch.float64, device=dev) for k, n in (("vr", 5), ("vc", 6), ("vf", 200), ("gr", 5), ("gc", 16), ("gf", 200))}
        torch.cuda.synchronize(dev)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.sync_visual_search(kp, ssearch, pairs, 0, initial_offset_ms=5.0, search_size_ms=6.0, result_ptr=d["vr"].data_ptr(), coarse_ptr=d["vc"].data_ptr(), fine_ptr=d["vf"].data_ptr())
        be.sync_gyro_search(ranges, 10.0, 8.0, result_ptr=d["gr"].data_ptr(), coarse_ptr=d["gc"].data_ptr(), fine_ptr=d["gf"].data_ptr())
        be.synchronize()
        h = {k: v.cpu().numpy() for k, v in d.items()}
    finally:
        be.close()
    for (r, c, f), name in ((("vr", "vc", "vf"), "visual search"), (("gr", "gc", "gf"), "gyro search")):
        res, coarse, fine = got[name]
        assert h[r].tobytes() == res.tobytes(), name
        assert same_bits(h[c], np.asarray(coarse).reshape(-1)) and same_bits(h[f], np.asarray(fine).reshape(-1)), name
