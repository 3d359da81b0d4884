"""The numpy statement of the gyro-match offset search (tests/_syncgyrostmt.py) held to what it is for: on planted clips — a smooth gyro (per axis four sinusoids,
0.3 - 4 Hz, 5 - 25 deg/s each) and estimated rates that are that gyro delayed by a planted offset — find_offsets returns the planted offset.

The bound is reasoned, not fitted: the coarse step is 1 ms, the fine stage looks only BELOW the coarse pick, and a lookup takes the NEXT gyro sample, so the search
can be off by up to 1 ms plus one gyro sample period.  Measured worst case per clip (fps, gyro Hz, planted ms -> error ms / bound ms), search_size 5000:
    25    200      0.00  3.99 / 6.00        30    500      7.30  0.69 / 3.00        50    800   -133.37  0.36 / 2.25        59.94 1000    412.60  0.22 / 2.00
    60   1600   -871.25  0.01 / 1.63       120   2000   1999.50  0.49 / 1.50        30   2000  -2000.00  0.01 / 1.50        60    200   1500.20  3.79 / 6.00
   120    500  -1234.56  0.55 / 3.00        25   1000      0.45  0.46 / 2.00        59.94  400     -0.77  0.76 / 3.50        50   2000   1000.00  0.01 / 1.50
"""
import numpy as np
import pytest

import _syncgyrostmt as G


@pytest.fixture(scope="module")
def found():
    out = []
    for i in range(len(G.PLANTED)):
        c = G.planted(i)
        ins = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 5000.0)
        out.append((c, ins, G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 5000.0)))
    return out


def test_the_planted_clips_cover_the_issue():
    assert len(G.PLANTED) >= 10
    assert {p[0] for p in G.PLANTED} == {25.0, 30.0, 50.0, 59.94, 60.0, 120.0}
    rates = [p[1] for p in G.PLANTED]
    assert min(rates) == 200.0 and max(rates) == 2000.0
    offs = [p[2] for p in G.PLANTED]
    assert 0.0 in offs and min(offs) == -2000.0 and max(offs) > 1999.0 and any(o < 0 for o in offs) and any(o > 0 for o in offs)


@pytest.mark.parametrize("i", range(len(G.PLANTED)))
def test_finds_the_planted_offset(found, i):
    clip, ins, offsets = found[i]
    assert len(ins) == 1 and len(offsets) == 1
    middle, value, cost = offsets[0]
    err, bound = abs(value - clip.offset_ms), 1.0 + 1000.0 / clip.rate
    print("fps %g, gyro %g Hz, planted %g ms: found %.2f, error %.3f ms (bound %.3f), cost %g" % (clip.fps, clip.rate, clip.offset_ms, value, err, bound, cost))
    assert err <= bound, (G.PLANTED[i], value, err, bound)
    assert middle == (clip.ranges[0][0] + (clip.ranges[0][1] - clip.ranges[0][0]) / 2.0) / 1000.0
    assert cost < G.F64_MAX


def test_estimated_rates_at_25_and_30_fps_are_never_filtered(found):
    """2 * 20 Hz > fps: Coefficients::from_params fails, the reference ignores it (essential_matrix.rs:47) and goes on with the unfiltered series; the gyro (>= 200 Hz)
    is always filtered"""
    for clip, ins, _ in found:
        assert ins[0]["gyro_filtered"] is True
        assert ins[0]["est_filtered"] is (clip.fps >= 40.0), clip.fps
        raw = np.array([clip.estimated_gyro[k][1] for k in sorted(clip.estimated_gyro) if clip.ranges[0][0] <= k < clip.ranges[0][1]])
        assert np.array_equal(raw, ins[0]["est"][:, 1:]) is (clip.fps < 40.0)


def test_a_clip_below_three_degrees_per_second_is_skipped():
    c = G.Clip(60.0, 1000.0, 12.0, seed=5, scale=0.02)
    assert G.max_angle(list(c.estimated_gyro.values())) < 3.0
    assert G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 5000.0) == []
    assert G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 5000.0) == []


def test_guards():
    c = G.planted(3)
    args = (c.duration_ms, c.fps, c.ranges, 0.0, 100.0)
    assert G.range_inputs({}, c.raw_imu, *args) == [] and G.range_inputs(c.estimated_gyro, [], *args) == []
    assert G.range_inputs(c.estimated_gyro, c.raw_imu, 0.0, c.fps, c.ranges, 0.0, 100.0) == []
    assert G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, [(5, 5), (9, 3), (30000000, 31000000)], 0.0, 100.0) == []      # empty, reversed, past the clip
    # the end of a range is excluded, its start included
    keys = sorted(c.estimated_gyro)
    r = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, [(keys[100], keys[130])], 0.0, 100.0)
    assert len(r[0]["est"]) == 30 and r[0]["est"][0, 0] == c.estimated_gyro[keys[100]][0] and r[0]["est"][-1, 0] == c.estimated_gyro[keys[129]][0]
    # the gyro window: ts + initial_offset within [first - search_size, last + search_size], both ends included
    g = r[0]["gyro"][:, 0]
    lo, hi = r[0]["est"][0, 0] - 100.0, r[0]["est"][-1, 0] + 100.0
    want = [t for t, _ in c.raw_imu if lo <= t + 0.0 <= hi]
    assert list(g) == want


def test_an_offset_beyond_ninety_percent_of_the_range_is_rejected():
    c = G.Clip(60.0, 1000.0, 950.0, seed=21)
    rejected = []
    assert G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 1000.0, rejected) == []
    assert len(rejected) == 1 and abs(rejected[0][1] - 950.0) <= 2.0                  # it was found, and turned away: |offset - initial| >= 0.9 * search_size
    kept = G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 1100.0)
    assert len(kept) == 1 and abs(kept[0][1] - 950.0) <= 2.0                          # 950 < 990


def test_the_median_rule():
    assert G.median([3.0]) == 3.0 and G.median([5.0, 1.0, 3.0]) == 3.0 and G.median([4.0, 1.0, 2.0, 10.0]) == 3.0
    offs = [(0.0, 10.0, 1.0), (1.0, -4.0, 1.0), (2.0, 7.0, 1.0), (3.0, 100.0, 1.0)]
    assert G.initial_offset_fast(offs, 1.5, 5000.0) == (8.5, 3000.0)
    assert G.initial_offset_fast([], 1.5, 5000.0) == (1.5, 5000.0)                    # nothing found: unchanged


def test_the_vectorised_costs_are_the_scalar_fold():
    c = G.planted(2)
    r = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 5000.0)[0]
    tree = G.Tree(r["gyro"], r["gyro_has"])
    cands = np.array([-5000.0, -4999.0, -133.37, -133.01, 0.0, 4998.5, 4999.0, 1e7, -1e7])
    got = G.costs(cands, r["est"], r["est_has"], tree)
    for k, offs in enumerate(cands):
        assert got[k] == G.cost_scalar(float(offs), r["est"], r["est_has"], tree), offs
    assert got[-2] < G.F64_MAX and got[-1] == G.F64_MAX             # every query negative: each lands on the first sample, a match; every query past the end: a miss


def test_key_and_find_min():
    assert [G.key(v) for v in (float("nan"), -1.0, -0.0, 0.99, 1.0, 2.9, 1e30, float("inf"))] == [0, 0, 0, 0, 1, 2, 2 ** 64 - 1, 2 ** 64 - 1]
    assert list(G.keys_of([float("nan"), -1.0, 0.99, 2.9, 1e30])) == [0, 0, 0, 2, 2 ** 64 - 1]
    assert G.find_min([3.0, 1.0, 2.0, 1.0, 5.0]) == 3 and G.find_min([G.F64_MAX] * 4) == 3 and G.find_min([1.0]) == 0
    assert len(G.coarse_candidates(0.0, 2.5)) == 4 and list(G.coarse_candidates(10.0, 2.5)) == [7.5, 8.5, 9.5, 10.5]       # the cast comes before the multiplication
    f = G.fine_candidates(100.0)
    assert len(f) == 200 and f[0] == 98.0 and f[-1] == 100.0 + (-2.0 + 199.0 * 0.01) and f[-1] < 100.0                     # below the coarse pick only


class StatementBackend:
    """a stand-in for warp.Backend: sync_gyro_search answered by the statement (the device's answers are held to it elsewhere)"""

    def __init__(self):
        self.calls = 0

    def sync_gyro_search(self, ranges, initial_offset_ms, search_size_ms):
        from gyroflow_amd import abi
        self.calls += 1
        out = []
        for est, est_has, gyro, gyro_has in ranges:
            s = G.search(est, est_has, gyro, gyro_has, initial_offset_ms, search_size_ms)
            out.append(abi.SyncResult(found=s["found"], n_coarse=s["n_coarse"], coarse_value=s["coarse_value"], coarse_cost=s["coarse_cost"], value=s["value"], cost=s["cost"]))
        return out


@pytest.mark.parametrize("i", [1, 3])
def test_the_python_mirrors_host_half_is_the_statements(i):
    """synchronization.essential_ranges (guards, range cut, gyro window, max-angle skip, gfw_lowpass_gyro) against range_inputs, to the bit — 30 fps unfiltered, 59.94 filtered"""
    from gyroflow_amd import synchronization as SY
    c = G.planted(i)
    keys = sorted(c.estimated_gyro)
    c.estimated_gyro[keys[len(keys) // 2 - 3]] = (c.estimated_gyro[keys[len(keys) // 2 - 3]][0], None)
    c.raw_imu[len(c.raw_imu) // 2] = (c.raw_imu[len(c.raw_imu) // 2][0], None)
    ranges = [(5, 5), c.ranges[0], (12000000, 12400000), (40000000, 41000000)]
    sp = SY.SyncParams(20.0, 700.0)
    got = SY.essential_ranges(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, sp)
    want = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, 20.0, 700.0)
    assert [k for k, _ in got] == [r["index"] for r in want] == [1, 2]
    for (_, (est, est_has, gyro, gyro_has)), r in zip(got, want):
        assert G.same_bits(est, r["est"]) and G.same_bits(gyro, r["gyro"])
        assert list(est_has) == list(r["est_has"]) and list(gyro_has) == list(r["gyro_has"])
        assert not all(est_has) or not all(gyro_has) or r["index"] == 2
    assert SY.essential_ranges({}, c.raw_imu, c.duration_ms, c.fps, ranges, sp) == [] and SY.essential_ranges(c.estimated_gyro, [], c.duration_ms, c.fps, ranges, sp) == []
    assert SY.essential_ranges(c.estimated_gyro, c.raw_imu, 0.0, c.fps, ranges, sp) == []


def test_the_python_mirrors_acceptance_rule_and_fast_initial_offset():
    from gyroflow_amd import synchronization as SY
    c = G.planted(3)                                                                   # planted 412.6 ms
    ranges = [c.ranges[0], (5, 5), (12000000, 13500000), (14000000, 15500000)]
    be = StatementBackend()
    sp = SY.SyncParams(0.0, 600.0)
    got = SY.find_offsets_essential(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, sp, be)
    assert be.calls == 1                                                               # all ranges in ONE search call
    want = G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, 0.0, 600.0)
    assert len(got) == 3 and G.same_bits(np.array(got), np.array(want))
    assert [m for m, _, _ in got] == [9750.0, 12750.0, 14750.0]
    assert SY.initial_offset_fast(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, sp, be) == (sorted(o for _, o, _ in got)[1], 3000.0)
    assert SY.median_offset([4.0, 1.0, 2.0, 10.0]) == 3.0 and SY.median_offset([2.0]) == 2.0
    narrow = SY.SyncParams(0.0, 440.0)                                                 # 412.6 >= 0.9 * 440: found, and turned away
    assert SY.find_offsets_essential(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, narrow, be) == []
    assert SY.initial_offset_fast(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, narrow, be) == (0.0, 440.0)           # nothing found: unchanged
    assert SY.initial_offset_fast(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, [], sp, be) == (0.0, 600.0)
    calls = be.calls
    assert SY.find_offsets_essential(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, [(5, 5)], sp, be) == [] and be.calls == calls      # nothing reaches the search: no call


def test_the_ring_slot_count_the_mirror_states_is_the_librarys():
    """abi.SYNC_GYRO_RING_SLOTS is what tests/test_gpu_sync_gyro.py sizes its 'one call more than the ring has slots' by: it must be gfw_ctx::kGyroSlots"""
    import os
    import re
    from gyroflow_amd import abi
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gyroflow_amd", "csrc", "gfw_api.hip")).read()
    m = re.search(r"kGyroSlots\s*=\s*(\d+)\s*;\s*\n\s*StagingRing<kGyroSlots>\s+gyro_ring;", src)
    assert m and int(m.group(1)) == abi.SYNC_GYRO_RING_SLOTS, m and m.group(0)
