"""TEST INFRASTRUCTURE: the point-pair calls (gfw_sync_visual_*, gfw_pose_almeida, gfw_pose_essential, gfw_sync_rs_*) on a pair set whose first point is not the
first entry of the caller's arrays — pair_first[0] = 3, three unused points in front of both arrays.  The pose calls and the visual search stage pair_first as given
and the arrays from their start, the rs-sync calls rebase to 0 and stage from pair_first[0] on; either way every output equals that of the same pairs at a base of
0 to the bit.  The smallest shapes that still run every stage, shared by the interpreter tier (tests/test_emu_*.py) and the device tier (tests/test_gpu_*.py)."""
import contextlib

import numpy as np

from gyroflow_amd import warp
import _posecase as PC
import _posesscase as EC
import _posessstmt as ES
import _rssynccase as RC
import _rssyncstmt as RS
import _synccase as SC
import _syncstmt as SS

LEAD = 3


@contextlib.contextmanager
def leading_points(n=LEAD):
    """Inside the block the flat arrays of every point-pair call (warp.Backend._sync_pairs packs them for the library and for the interpreter alike) start with
    `n` unused points and pair_first with n"""
    plain = warp.Backend._sync_pairs

    def packed(pairs):
        ts, first, pa, pb = plain(pairs)
        unused = np.full((n, 2), 12345.5, dtype=np.float32)
        return ts, first + np.int32(n), np.ascontiguousarray(np.concatenate([unused, pa])), np.ascontiguousarray(np.concatenate([-unused, pb]))
    warp.Backend._sync_pairs = staticmethod(packed)
    try:
        yield
    finally:
        warp.Backend._sync_pairs = staticmethod(plain)


def same_bits(got, want, what):
    """every array of two results' (nested) tuples, bit for bit"""
    if isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, "%s[%d]" % (what, i))
        return
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), "%s differs between a base of 0 and a base of %d" % (what, LEAD)


def assert_base_does_not_matter(call, what):
    """call() -> arrays (nested tuples of them): once as the pairs are, once behind the unused points"""
    want = call()
    with leading_points():
        ts, first, pa, pb = warp.Backend._sync_pairs([(0, 1, np.zeros((2, 2)), np.ones((2, 2)))])
        assert first.tolist() == [LEAD, LEAD + 2] and first.dtype == np.int32 and pa.shape == (LEAD + 2, 2) and pb.dtype == np.float32      # the block does what it says
        got = call()
    same_bits(got, want, what)
    return want


_CASES = {}


def _once(name, make):
    if name not in _CASES:
        _CASES[name] = make()
    return _CASES[name]


def almeida():
    """pairs of 3 and 5 points, 4 rounds"""
    return _once("almeida", lambda: PC.Case("base-offset", PC.tele_fisheye_clip(), [3, 5], 4))


def essential():
    """pairs of 8 and 9 points, 4 rounds"""
    return _once("essential", lambda: EC.Case("base-offset", PC.tele_fisheye_clip(), [8, 9], 4))


class RsCall:
    """one range of two 8-point pairs, a 16-sample track around them (6 ms apart), 3 candidates; and a search of 1 round whose round 0 has 3 candidates"""

    def __init__(self):
        self.cam = ES.Camera(EC.pinhole_clip(), RC.FLOW)
        self.cfg = RS.Cfg(readout_ms=12.0, rounds=1)
        self.ranges = [RC.plant_range(self.cam, [8, 8], 0.0033, 12.0, RC.unit((1.0, 0.4, 0.2), 0.5), 5, start_s=0.004)]
        ts = np.arange(16, dtype=np.int64) * 6000                             # 0 .. 90 ms: the frames of both pairs (4, 37.3, 70.7 ms) and their rows lie inside
        self.track = (ts, np.ascontiguousarray(RC.quat_true(ts / 1000000.0)))
        self.candidates = [[0.0, 0.003, 0.006]]
        self.initial_s, self.radius_s = 0.003, self.cfg.step_s                # h = 1: 3 candidates


def rs_sync():
    return _once("rs", RsCall)


def visual():
    """-> (Range of two 4-point pairs, 3 candidates)"""
    def make():
        rng, _ = SC.planted("fisheye-r12", "emu", 0)
        pairs = [(a, b, p[:4], q[:4]) for a, b, p, q in rng.pairs[1:3]]
        return SS.Range(rng.clip, pairs), [(0.0, 12.0), (SC.OFFSET, 12.0), (11.0, 0.0)]
    return _once("visual", make)
