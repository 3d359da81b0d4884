"""TEST INFRASTRUCTURE: the ranges the sync search is tested on (statement, host-interpreted kernels, device alike) and the arguments of gfw_sync_visual_* for them.

Six planted clips (tests/_syncstmt.py: PlantedClip, planted_pairs), 320 x 180: the scene is seen through the gyro track delayed by OFFSET ms, with the clip's readout
time; matched frames are two frames apart at 30 fps (visual_features.rs:21, `next_frame_no = 2`).  track_scale = 14: calculate_distance truncates every squared
distance to an integer (`dist as u64`), so at this frame size (f = 150 px) a candidate 1 ms off the truth must move the points by more than a pixel for the coarse
stage to tell it from the truth.  Measured with the statement: at track_scale 3 every offset within 1 ms of the truth costs 0; at 10 the offset search meets the
condition but the readout search (a readout time moves a point's time by at most half of itself) picks a coarse candidate 1 ms off for two of four track seeds; at
14 all twelve searches pick the coarse candidate nearest the truth (tests/test_sync_statement.py asserts the condition itself).  The generic-model lens is the sony
polynomial and the digital lens the stretch: with this much rotation the planted source points lie far outside the frame, where poly5 / ptlens / opencv_standard and
the GoPro superview family are not inverted by their own inverse (the planted points would not map back onto the scene).

Three shapes of a range: "stmt" 4 pairs of 60 .. 200 points; "gpu" 6 pairs of 1, 10, 63, 64, 65 and 200 points (under, at and over a wave); "emu" 3 small pairs.
The statement's costs of every candidate both stages visit are stored in tests/golden/sync_statement_costs.json (tests/golden/sync_statement_costs.py makes them:
minutes of Python for the rolling-shutter ranges); tests/test_sync_statement.py re-derives a sample of them on every run."""
import json
import os

import numpy as np

from gyroflow_amd import abi
import _syncstmt as SS
import _zoomstmt as Z

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OFFSET = 7.3                    # the planted gyro delay, ms (mode 0 searches it; mode 1 ranges have none)
GAP_MS = 1000.0 / 30.0 * 2.0
SHAPES = {"stmt": [60, 100, 140, 200], "gpu": [1, 10, 63, 64, 65, 200], "emu": [1, 10, 65]}
TIMES = [1200.0, 1500.0, 1900.0, 2300.0, 2700.0, 3100.0]
# (mode 0: initial_offset, search_size — 40 coarse candidates, 4 for the interpreter; mode 1: scaled_fps — 2 * 20 coarse candidates, 2 * 2 for the interpreter)
SEARCH = {"stmt": (0.0, 40.0, 50.0), "gpu": (0.0, 40.0, 50.0), "emu": (6.0, 4.0, 500.0)}


def clips():
    size = (320, 180)
    return [SS.PlantedClip("fisheye-r0", track_scale=14.0),
            SS.PlantedClip("fisheye-r12", readout=12.0, track_scale=14.0),
            SS.PlantedClip("readout-neg", readout=-12.0, track_scale=14.0),
            SS.PlantedClip("readout-horizontal", readout=12.0, horizontal=True, track_scale=14.0),
            SS.PlantedClip("sony-r0", lens=Z.physical_lens("sony", size), track_scale=14.0, seed=13),
            SS.PlantedClip("digital-lens", digital="digital_stretch", digital_params=[1.1, 0.95], track_scale=14.0)]


CLIPS = {c.name: c for c in clips()}
_RANGES = {}


def planted(name, shape, mode):
    """-> (Range, q per pair): mode 0 plants OFFSET and the clip's readout time, mode 1 no offset and the clip's readout time (the value it searches)"""
    key = (name, shape, mode)
    if key not in _RANGES:
        clip = CLIPS[name]
        n = SHAPES[shape]
        pairs, qs = SS.planted_pairs(clip, OFFSET if mode == 0 else 0.0, clip.readout, n, TIMES[:len(n)], seed=5 + mode, gap_ms=GAP_MS)
        _RANGES[key] = (SS.Range(clip, pairs), qs)
    return _RANGES[key]


def truth(name, mode):
    return OFFSET if mode == 0 else CLIPS[name].readout


def search_args(name, shape, mode):
    """keyword arguments of _syncstmt.search / Backend.sync_visual_search for the case"""
    initial, size, fps = SEARCH[shape]
    if mode == 0:
        return dict(initial_offset=initial, search_size=size, readout=CLIPS[name].readout)
    return dict(fps=fps)


def sync_search(clip, use_sync_offsets=0):
    """abi.SyncSearch of a statement clip (output size = source size, fov 1)"""
    s = abi.SyncSearch(width=clip.size[0], height=clip.size[1], horizontal_readout=1 if clip.horizontal else 0, use_sync_offsets=int(use_sync_offsets),
                       video_rotation_deg=clip.video_rotation)
    for i, v in enumerate(np.asarray(clip.new_k(), dtype=np.float64).reshape(9)):
        s.new_k[i] = v
    return s


def case_key(name, shape, mode):
    return "%s/%s/%d" % (name, shape, mode)


_GOLD = {}


def stored(name, shape, mode):
    """the statement's search of the case as stored: dict(coarse_costs, coarse_pick, fine_costs, fine_pick, value, cost)"""
    if not _GOLD:
        _GOLD.update(json.load(open(os.path.join(GOLDEN, "sync_statement_costs.json")))["cases"])
    return _GOLD[case_key(name, shape, mode)]


def sensitivity():
    return json.load(open(os.path.join(GOLDEN, "sync_rotation_sensitivity.json")))["clips"]


def stage_candidates(name, shape, mode, coarse_value=None):
    """the candidates [(offs, readout)] of the coarse stage, or of the fine stage around `coarse_value`"""
    a = search_args(name, shape, mode)
    if coarse_value is None:
        return SS.coarse_candidates(mode, a.get("initial_offset", 0.0), a.get("search_size", 0.0), a.get("readout", 0.0), a.get("fps", 30.0))
    return SS.fine_candidates(mode, coarse_value, a.get("readout", 0.0))
