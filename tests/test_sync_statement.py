"""The host statement of the visual-features sync search (tests/_syncstmt.py) held to what the search is for, before anything is compared with it: it finds a
planted gyro delay (mode 0) and a planted frame readout time (mode 1).

The ranges are tests/_synccase.py's "stmt" shape — 320 x 180, 4 pairs of 60, 100, 140 and 200 points — over six clips: fisheye without and with a 12 ms readout,
a negative readout, a horizontal readout, one generic-model lens (sony), a digital lens (stretch).  The scene: output-grid points q; p1 = the render's forward map of q (the
oracle's undistort_coord over _hoststmt.row_matrices_from_tracks) at ts_A - d, p2 likewise at ts_B - d, for a clip whose smoothing target is constant, so both frames
share a world frame.  The issue words this "a constant smoothed track"; the track a GyroSource STORES as smoothed is the correction sq^-1 * q
(gyro_source/mod.rs:682-684), so the constant target is the stored track equal to the original one (_syncstmt.PlantedClip) — a constant stored track would make the
rotation of a frame without rolling shutter independent of the offset, and the search blind.

With rolling shutter the plant iterates a point's row time to its fixed point (_syncstmt.planted_pairs says why).

Motion amplitude: track_scale 14 (tests/_synccase.py says why: `dist as u64` truncates, the frame is small).  With it the structural condition holds on all twelve
searches: the coarse pick is the candidate nearest the truth (0.3 ms off for the offset, exact for the readout time), so the fine stage ([-1, +0.99] ms around the
pick) contains the truth.

Measured with the statement on the CPU (profiles/sync_search.txt): the worst error of the final value is 0.70 ms (sony-r0, readout search: truth 0, found 0.70);
the offset searches end 0.29 .. 0.42 ms off, the readout searches 0.43 .. 0.70 ms — squared distances below one pixel^2 all truncate to 0, so a stretch of candidates
around the truth costs 0 and the LAST of them wins.  Asserted at twice that, capped at 1 ms: 1 ms.

The costs of the rolling-shutter searches are minutes of Python, so the searches are read from tests/golden/sync_statement_costs.json (made by this statement:
tests/golden/sync_statement_costs.py); every test re-derives a sample of the stored costs, and the two searches without rolling shutter that are cheap run whole."""
import numpy as np
import pytest

import _synccase as SC
import _syncstmt as SS

WORST_MEASURED_MS = 0.70
BAR_MS = min(2.0 * WORST_MEASURED_MS, 1.0)
CASES = [(n, m) for n in sorted(SC.CLIPS) for m in (0, 1)]


@pytest.mark.parametrize("name,mode", CASES)
def test_planted_points_map_back_onto_the_scene(name, mode):
    """at the true parameters p1 and p2 land within a fraction of a pixel of q (exactly the render's inverse without rolling shutter; with it the render picks a
    row's matrix by the row it lands in, the point map by the point's own row)"""
    rng, qs = SC.planted(name, "stmt", mode)
    m = SS.mapped_points(rng, SC.OFFSET if mode == 0 else 0.0, rng.clip.readout)
    q = np.concatenate(qs)
    err = max(float(np.max(np.abs(m[:, 0] - q))), float(np.max(np.abs(m[:, 1] - q))))
    print("%s mode %d: planted points map back within %.4f px" % (name, mode, err))
    assert err < 0.25, (name, mode, err)


@pytest.mark.parametrize("name,mode", CASES)
def test_search_finds_the_planted_value(name, mode):
    rng, _ = SC.planted(name, "stmt", mode)
    st = SC.stored(name, "stmt", mode)
    col = 0 if mode == 0 else 1
    coarse = SC.stage_candidates(name, "stmt", mode)
    fine = SC.stage_candidates(name, "stmt", mode, coarse[st["coarse_pick"]][col])
    truth = SC.truth(name, mode)
    if rng.clip.readout == 0.0 and mode == 0:                                     # cheap: the whole search, live
        live = SS.search(rng, mode, **SC.search_args(name, "stmt", mode))
        assert {k: live[k] for k in st} == st, name
    else:                                                                         # a sample of the stored costs, live
        for i in (0, st["coarse_pick"], len(coarse) - 1):
            assert SS.cost(rng, *coarse[i]) == st["coarse_costs"][i], (name, mode, i)
        for i in (0, st["fine_pick"], 199):
            assert SS.cost(rng, *fine[i]) == st["fine_costs"][i], (name, mode, i)
    assert len(st["coarse_costs"]) == 40 and len(st["fine_costs"]) == 200
    assert st["coarse_pick"] == SS.find_min(st["coarse_costs"]) and st["fine_pick"] == SS.find_min(st["fine_costs"])
    assert st["value"] == fine[st["fine_pick"]][col] and st["cost"] == st["fine_costs"][st["fine_pick"]]
    picked = coarse[st["coarse_pick"]][col]
    print("%s mode %d: truth %.2f, coarse pick %.0f, found %.2f (error %.2f ms), cost %g" % (name, mode, truth, picked, st["value"], abs(st["value"] - truth), st["cost"]))
    assert abs(picked - truth) < 1.0, (name, mode, picked, truth)                 # the structural condition
    assert abs(st["value"] - truth) <= BAR_MS, (name, mode, st["value"], truth)
    assert max(st["coarse_costs"]) > st["cost"]                                   # the landscape is not flat


def test_fold_as_written():
    """:66-81 on small hand-made sets"""
    pts = lambda *d: (np.array([[10.0, 10.0]] * len(d), np.float32), np.array([[10.0 + x, 10.0] for x in d], np.float32))
    assert SS.fold(*pts(), 320, 180) == 0
    assert SS.fold(*pts(3.0), 320, 180) == 0                                      # (1 as f64 * 0.9) as usize = 0
    assert SS.fold(*pts(*[3.0] * 10), 320, 180) == 81                             # 9 of 10
    assert SS.fold(*pts(1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0), 320, 180) == sum(x * x for x in range(1, 10))
    assert SS.fold(*pts(*[1.9] * 10), 320, 180) == 27                             # 3.61 as u64 = 3
    a, b = pts(*[2.0] * 10)
    a[0] = (0.0, 10.0); a[1] = (10.0, 180.0); b[2] = (320.0, 10.0); b[3] = (-1000000.0, -1000000.0)
    assert SS.fold(a, b, 320, 180) == 4 * 5                                       # six valid, k = 5
    assert SS.find_min([3.0, 1.0, 2.0, 1.0, 5.0]) == 3 and SS.find_min([]) is None and SS.find_min([0.0, 0.0]) == 1


def test_find_offsets_applies_the_acceptance_rule(monkeypatch):
    rng, _ = SC.planted("fisheye-r0", "stmt", 0)
    st = SC.stored("fisheye-r0", "stmt", 0)
    found = SS.find_offsets(lambda a, b: rng, [(1000000, 3400000)], 0, **SC.search_args("fisheye-r0", "stmt", 0))
    assert found == [(2200.0, st["value"], st["cost"])]
    # :137 — `(lowest.0 - initial_offset).abs() < search_size * 0.9`; the readout search has no such rule and reports timestamp 0
    for value, kept in ((3.0 + 1.79, True), (3.0 - 1.79, True), (3.0 + 1.81, False), (3.0 - 1.81, False)):
        monkeypatch.setattr(SS, "search", lambda *a, **k: dict(value=value, cost=5.0))
        assert SS.find_offsets(lambda a, b: rng, [(0, 1000)], 0, initial_offset=3.0, search_size=2.0) == ([(0.5, value, 5.0)] if kept else [])
        assert SS.find_offsets(lambda a, b: rng, [(0, 1000)], 1, fps=50.0) == [(0.0, value, 5.0)]
    monkeypatch.setattr(SS, "search", lambda *a, **k: None)
    assert SS.find_offsets(lambda a, b: rng, [(0, 1000)], 0, initial_offset=3.0, search_size=0.5) == []


def test_python_mirror_selects_pairs_and_applies_the_rule():
    """gyroflow_amd.synchronization.find_offsets_visual over a stand-in backend: which pairs a range takes (:32-47), the middle timestamp, the 90 % rule, for_rs"""
    from gyroflow_amd import abi, stabilization as ST, synchronization as SY
    clip = SC.CLIPS["fisheye-r12"]
    cp = ST.ComputeParams(clip.lens, width=320, height=180, output_width=320, output_height=180, frame_readout_time=12.0, scaled_fps=50.0)
    pts = lambda n: np.zeros((n, 2), np.float32)
    matched = {100: (166, pts(3), pts(3)), 200: (266, pts(0), pts(0)), 300: (366, pts(4), pts(5)), 400: (466, pts(2), pts(2)), 1000: (1066, pts(1), pts(1))}
    calls = []

    class Backend:
        def sync_visual_search(self, kp, search, pairs, mode, initial_offset_ms=0.0, search_size_ms=0.0, frame_readout_time_ms=0.0, scaled_fps=30.0):
            calls.append(([p[0] for p in pairs], mode, search.use_sync_offsets, initial_offset_ms, search_size_ms, frame_readout_time_ms, scaled_fps))
            return abi.SyncResult(found=1 if pairs else 0, n_coarse=10, value=initial_offset_ms + (8.0 if len(pairs) == 1 else 9.5), cost=7.0)
    got = SY.find_offsets_visual(cp, [(100, 1000), (1000, 2000), (5000, 6000)], matched, SY.SyncParams(2.0, 10.0), Backend())
    assert got == [(1.5, 10.0, 7.0)]                                              # range 1: 9.5 away, not < 9; range 3: nothing found
    assert calls == [([100, 400], 0, 0, 2.0, 10.0, 12.0, 30.0), ([1000], 0, 0, 2.0, 10.0, 12.0, 30.0), ([], 0, 0, 2.0, 10.0, 12.0, 30.0)]
    del calls[:]
    got = SY.find_offsets_visual(cp, [(100, 1000)], matched, SY.SyncParams(2.0, 10.0), Backend(), for_rs=True)
    assert got == [(0.0, 9.5, 7.0)] and calls == [([100, 400], 1, 1, 0.0, 0.0, 0.0, 50.0)]
    kp, search = SY.search_inputs(cp)
    assert list(search.new_k) == list(np.asarray(clip.new_k()).reshape(9)) and kp.lens_correction_amount == 1.0 and (search.width, search.height) == (320, 180)
