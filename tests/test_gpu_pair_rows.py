"""The pair's second matrix row on the device (gfw_frame.hip, GFW_PAIR_ROW: fetched only by the lanes whose two rows differ, under their exec mask; a wave without
such a lane branches over the fetch).  The clips of tests/test_emu_pair_rows.py at 320 x 192, twelve frames in one clip call: the specialised kernel as shipped, the
same library with GFW_JIT_DEFS=GFW_PAIR_ROW=0 (two unconditional fetches) and the ahead-of-time kernel (GFW_OPT_JIT 0) must each write the oracle's bytes.  Which
regime a clip is in — no pair differs, a third, nearly all — is asserted from the oracle's first pass.  One full-size C2 frame through a clip call must leave what
the reference's own kernel wrote (tests/golden/ref_golden.json)."""
import contextlib
import json
import os
import zlib

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
import _pair_rows as P

pytestmark = pytest.mark.gpu

W, H, N = 320, 192, 12
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_golden.json")))
_clips = {}


def clip(case, w=W, interp=2):
    """-> frames, the oracle's planes per frame (built once per clip, shared by the runs and left unchanged)"""
    key = (case, w, interp)
    if key not in _clips:
        frames = [P.case_frame(case, "YUV422P16LE", w, H, f, interp=interp) for f in range(N)]
        refs = [O.run_frame(fr) for fr in frames]
        for ref in refs:
            for p in ref:
                p.setflags(write=False)
        _clips[key] = (frames, refs)
    return _clips[key]


@contextlib.contextmanager
def jit_defs(value):
    """further definitions for the specialised kernels built inside (read by the library when it puts a clip's build together; part of the build's key)"""
    old = os.environ.get("GFW_JIT_DEFS")
    if value:
        os.environ["GFW_JIT_DEFS"] = value
    else:
        os.environ.pop("GFW_JIT_DEFS", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GFW_JIT_DEFS", None)
        else:
            os.environ["GFW_JIT_DEFS"] = old


def run_clip(frames, jit, defs="", device_src=False):
    """one gfw_undistort_clip over `frames` -> ([plane bytes] per frame, backend name)"""
    import torch
    dev = torch.device("cuda", 0)
    d_src = [fr.device_planes(dev) if device_src else [torch.from_numpy(pl["src"]).to(dev) for pl in fr.planes] for fr in frames]
    d_dst = [fr.device_outputs(dev) for fr in frames]
    d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [pl["params"] for pl in frames[0].planes]
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(), d_dst[j][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
    with jit_defs(defs):
        be = warp.Backend(params[0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
        try:
            be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            be.set_option(abi.OPT_SYNCHRONOUS, 0)
            be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
            be.set_option(abi.OPT_JIT, jit)
            warp.ClipCall(be, bufs, params, types, [m.data_ptr() for m in d_mat], frames[0].matrices.shape[0])()
            be.synchronize()
            backend = warp.last_backend()
        finally:
            be.close()
    torch.cuda.synchronize(dev)
    return [[t.cpu().numpy() for t in d_dst[j]] for j in range(len(frames))], backend


def check(case, w=W, interp=2):
    frames, refs = clip(case, w, interp)
    for jit, defs in ((2, ""), (2, "GFW_PAIR_ROW=0"), (0, "")):
        got, backend = run_clip(frames, jit, defs)
        tag = "%s %dx%d interpolation %d, jit %d [%s] (%s)" % (case, w, H, interp, jit, defs, backend)
        assert backend.startswith("yuv_fused") and backend.endswith("_jit") == (jit == 2), tag
        for f in range(len(frames)):
            for p, (a, b) in enumerate(zip(refs[f], got[f])):
                assert np.array_equal(a, b), "%s frame %d plane %d: %d bytes differ from the oracle" % (tag, f, p, int(np.count_nonzero(a != b)))


def test_no_pair_differs_the_wave_skips_the_fetch():
    """(b) rolling shutter over a flat first pass"""
    frames, _ = clip("flat")
    assert frames[0].matrices.shape[0] == 2 * H
    for pairs, quads, waves in P.clip_shares(frames):
        assert pairs == 0.0 and waves == 0.0
    check("flat")


def test_a_rolled_frame_lanes_on_both_sides():
    """(c) 25 degrees of roll: a third of the pairs, nine waves in ten"""
    for pairs, quads, waves in P.clip_shares(clip("roll")[0]):
        assert 0.05 < pairs < 0.95 and waves > 0.9, (pairs, quads, waves)
    check("roll")


def test_horizontal_rolling_shutter_nearly_every_pair_differs():
    """(d) the row index follows x"""
    for pairs, quads, waves in P.clip_shares(clip("hrs")[0]):
        assert pairs > 0.9 and waves == 1.0, (pairs, quads, waves)
    check("hrs")


def test_a_width_that_is_no_multiple_of_the_tile():
    """(f) 392 columns: three whole tiles and one whose wave has 60 dead lanes"""
    for pairs, quads, waves in P.clip_shares(clip("roll", w=392)[0]):
        assert 0.05 < pairs < 0.95
    check("roll", w=392)


@pytest.mark.parametrize("interp", [4, 8])
def test_bicubic_and_lanczos4_on_the_rolled_frame(interp):
    """(g) the LUT samplers keep their six unconditional fetches (the switch is compiled for bilinear only): either value of it leaves the oracle's bytes"""
    check("roll", interp=interp)


def test_a_full_size_c2_frame_is_the_reference_kernels():
    """the bench's first frame (seed 0x9F10) through a one-frame clip call, switch on and off: the CRCs of what the reference's own kernel wrote"""
    fr = S.SyntheticFrame("YUV422P16LE", 3840, 2160, seed=0x9F10, pixels=False)
    for defs in ("", "GFW_PAIR_ROW=0"):
        got, backend = run_clip([fr], 2, defs, device_src=True)
        assert backend == "yuv_fused_p1_jit", backend
        assert [zlib.crc32(p.tobytes()) for p in got[0]] == GOLD["c2_yuv422p16_3840x2160_rs"]["planes"], defs
