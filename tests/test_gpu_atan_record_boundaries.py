"""The arctangent of the branch-free row (gfw_frame.hip rd_lean_nobranch) where its reduction records meet: a wave whose lanes are all below 0.4375 skips the
reduction, every other wave reads each lane's record — r in [0.4375, 0.6875), [0.6875, 1.1875), ... — from LDS by a key of r's bit pattern.  Frames placed so that
every wave lies inside record 1, so that the 0.6875 circle cuts every wave of the left half, and so that the 0.4375 circle does: bit for bit the oracle's, from the
specialised and the ahead-of-time kernels.  (The placements were chosen for round 7's wave-uniform reduction — a record's constants as literals when a whole wave
shares it — which measured slower and was removed: profiles/r07_row_memops.txt; they guard the boundaries for whoever tries again.)

A wave is a strip of 128 x 1 luma pixels; the frame is 256 x 32 (two waves per row).  At fov 0.1 the output focal length is ten times the lens's, so r grows by
only 0.115 along a strip, and translation2d slides the frame along r.  Each placement's claim is checked here on the CPU first, from the frame's own matrices: r of
every pixel under EVERY row's matrix (the row a pixel takes is the first pass's business) gives bounds that hold whichever row is taken."""
import numpy as np
import pytest

from gyroflow_amd import synthetic as S, warp
import _oracle as O
from test_gpu_parity import assert_plane_equal

pytestmark = pytest.mark.gpu

W, H = 256, 32


def frame_at(t2x):
    return S.SyntheticFrame("YUV422P16LE", W, H, seed=0x51, fov=0.1, base_overrides={"translation2d": (t2x, 0.0)})


def r_bounds(fr, t2x):
    """-> (lo, hi)[H][W]: the least and the largest r = |(X / W, Y / W)| of each output pixel over the rows of the frame's matrix table"""
    x = np.arange(W, dtype=np.float64)[None, :] + t2x
    y = np.arange(H, dtype=np.float64)[:, None]
    lo, hi = np.full((H, W), np.inf), np.zeros((H, W))
    for m in fr.matrices.astype(np.float64):
        wd = x * m[6] + y * m[7] + m[8]
        r = np.hypot((x * m[0] + y * m[1] + m[2]) / wd, (x * m[3] + y * m[4] + m[5]) / wd)
        lo, hi = np.minimum(lo, r), np.maximum(hi, r)
    return lo, hi


def strips(a):
    return [a[:, :128], a[:, 128:]]


def check(fr, what):
    ref = O.run_frame(fr)
    luma = np.frombuffer(ref[0], np.uint16)
    assert np.count_nonzero(luma) > 0.9 * W * H, "%s: the frame shows the source (not the background), so a wrong arctangent moves pixels" % what
    for jit in (2, 0):
        got = warp.run_frame(fr, jit=jit)
        assert warp.last_backend().endswith("_jit") == (jit == 2), (what, warp.last_backend())
        for i, (a, b) in enumerate(zip(ref, got)):
            assert_plane_equal(a, b, fr.planes[i]["pixel_type"], "%s: jit %d, plane %d" % (what, jit, i))


def test_every_wave_inside_one_record():
    fr = frame_at(687.0)
    lo, hi = r_bounds(fr, 687.0)
    assert lo.min() >= 0.4375 + 0.005 and hi.max() < 0.6875 - 0.005, (lo.min(), hi.max())           # record 1 everywhere
    check(fr, "record 1 everywhere")


def test_the_0_6875_circle_crosses_the_left_strip():
    fr = frame_at(905.0)
    lo, hi = r_bounds(fr, 905.0)
    (l0, l1), (h0, h1) = strips(lo), strips(hi)
    assert np.all(h0.min(axis=1) < 0.6875 - 0.02) and np.all(l0.max(axis=1) >= 0.6875 + 0.02) and l0.min() >= 0.4375       # every wave of the left strip: records 1 and 2
    assert l1.min() >= 0.6875 + 0.005 and h1.max() < 1.1875                                                                    # the right strip: record 2 alone
    check(fr, "records 1 | 2")


def test_the_0_4375_circle_crosses_the_left_strip():
    fr = frame_at(602.0)
    lo, hi = r_bounds(fr, 602.0)
    (l0, l1), (h0, h1) = strips(lo), strips(hi)
    assert np.all(h0.min(axis=1) < 0.4375 - 0.02) and np.all(l0.max(axis=1) >= 0.4375 + 0.02) and h0.max() < 0.6875       # every wave of the left strip: small angle and record 1
    assert l1.min() >= 0.4375 + 0.005 and h1.max() < 0.6875                                                                  # the right strip: record 1 alone
    check(fr, "small angle | record 1")
