"""TEST INFRASTRUCTURE: the case table of the sync-point choice (gyroflow_amd/csrc/gfw_sync_optim.hip: the max, rank, nms, pick and gather kernels behind the spectrum
stage) on TABULATED windows, shared by the statement's own tests (tests/test_optim_case_statement.py), the interpreter tier (tests/test_emu_optim_edges.py) and the
GPU tier (tests/test_gpu_optim_edges.py), so that all three run identical inputs against one f32 statement per case (tests/_syncoptimstmt.run_f32).

The identity it rests on: for a sample rate in [15.5, 16.5) fft_size = round(rate) = 16 = the hop, so the windows do not overlap, window i is samples 16 i .. 16 i + 15
and its band energies and rank depend on those 16 samples alone.  At 16.0 exactly ratio = 1.0 s (window times are exact integers), nms_radius = 4 and the bins are
[0, 2, 7, 7]: hf is empty.  A clip is laid out window by window from a small palette of 16-sample blocks — the three-phase 4 Hz tone (period 4 samples) at a handful of
amplitudes, a DC offset for lf, zeros, specials — so its rank profile is chosen in advance and equal blocks give bit-equal ranks.  The hf band needs a rate at which it is
not empty: 128.0 (bins [0, 2, 30, 63]) with a signal whose period divides 16 samples (8 Hz for mf, 32 Hz for hf), so that every window holds the same samples.

A case is plain data — gyro [3][S] f64, rate, target, trim ranges — plus the branch it exists for (`branch`), the wrong variants of the device's algorithm that must
change it (`broken_by`: tests/test_optim_case_statement.py) and a precondition `pre(s, c)` asserted on the f32 STATEMENT (rank order, equality of plateaus as uint32 views,
counts of NaN, cleared and surviving windows, which formula was taken) before any kernel output is read: `reference(name)` -> the statement's dict, computed once per
process and read-only.  A case that leaves its precondition gets other inputs, not another precondition.  Nothing here calls the library when the module is imported
(a test process must be free to load the GPU runtime in its own order): the trip-point cases, whose amplitudes come from the statement and so from the library's tables,
get their samples on first use — `case(name)` — and the exact hits, which exist or not, are listed by `exact_names()`.  Amplitudes that must straddle a trip point are FOUND by
bisection over the f32 amplitudes on the statement (`straddle`) and asserted to be neighbours on either side; an exact hit on the constant, where one exists, is a third
case.

What the identity does NOT cover: overlapping windows and the spectrum's arithmetic on real signals — those stay with the noise and planted clips
(tests/test_emu_sync_optim.py, tests/test_gpu_sync_optim.py)."""
import collections
import functools
import math

import numpy as np

import _syncoptimstmt as S

F32 = np.float32
R16 = 16.0
ALL = ((0.0, 1e9),)
LOW, MID, HIGH, TOP = 1.0, 2.0, 3.0, 6.0                      # tone amplitudes; a rank is about 139 per unit
NAN, INF = float("nan"), float("inf")
TARGET_MAX, TRIM_MAX = 65535, 1024                            # SYNC_OPTIM_TARGET_MAX, SYNC_OPTIM_TRIM_MAX (held to gyroflow_amd.abi by tests/test_optim_case_statement.py)

Case = collections.namedtuple("Case", "group branch gyro rate target trims broken_by pre")


# ---- the palette ----------------------------------------------------------------------------------------------------------------------------------------
def tone(amp, freq=4.0, rate=R16, n=16):
    """[3][n]: one oscillation seen by the three axes a third of a period apart, from t = 0"""
    t = np.arange(n) / rate
    return np.stack([amp * np.sin(2.0 * math.pi * freq * t + a * 2.0 * math.pi / 3.0) for a in range(3)])


def dc(level, amp=0.0):
    return np.full((3, 16), float(level)) + tone(amp)


ZERO = np.zeros((3, 16))


def poked(block, axis, sample, value):
    b = np.array(block, dtype=np.float64)
    b[axis, sample] = value
    return b


def lay(blocks):
    """the clip whose window i is blocks[i]; a number stands for the tone of that amplitude (0: zeros)"""
    return np.concatenate([(ZERO if b == 0 else tone(b)) if np.isscalar(b) else b for b in blocks], axis=1)


def profile(n, at, fill=0):
    """n windows of `fill` with {window: block or amplitude} laid over them"""
    blocks = [fill] * n
    for i, b in at.items():
        blocks[i] = b
    return lay(blocks)


def statement(gyro, rate, target, trims):
    with np.errstate(all="ignore"):                                                  # 1e300 `as f32`, inf - inf, NaN compares: ordinary input here
        return S.run_f32(gyro, rate, target, trims)


# ---- trip points, found on the statement ------------------------------------------------------------------------------------------------------------------
def straddle(f, lo, hi, trip):
    """-> (a, b, exact): neighbouring f32 values a < b with f(a) < trip <= f(b), by bisection over the f32 between lo and hi; exact: f(b) == trip.  Needs no
    monotonicity: the bisection keeps f(a) < trip <= f(b) and ends on neighbours"""
    a, b = np.array([lo, hi], dtype=F32).view(np.uint32).astype(np.int64)
    as_f = lambda u: float(np.array([u], dtype=np.uint32).view(F32)[0])
    assert 0 < a < b and f(as_f(a)) < trip <= f(as_f(b)), (lo, hi, trip)
    while b - a > 1:
        m = (a + b) // 2
        if f(as_f(m)) < trip:
            a = m
        else:
            b = m
    fa, fb = f(as_f(a)), f(as_f(b))
    assert b - a == 1 and fa < trip <= fb, (fa, fb)
    return as_f(a), as_f(b), bool(fb == trip)


def trip_clip(kind, x):
    """(gyro, rate): the clip in which amplitude x decides `kind`.  Every other window is fixed, far enough from window 2 that the suppression does not reach it"""
    if kind == "rank50":          # window 2's rank against 50 under the normal formula (window 8 keeps mf_max above 50)
        return profile(10, {2: x, 8: HIGH}), R16
    if kind == "mfmax50":         # window 2 holds the clip's largest mf; windows 5 and 8 carry lf, which only the low-motion formula adds
        return profile(10, {2: x, 5: dc(1.5, 0.1), 8: dc(1.0, 0.05)}), R16
    if kind == "lf650":           # window 2's lf against 650 under the normal formula
        return profile(10, {2: dc(x, MID), 8: HIGH}), R16
    assert kind == "hf450"        # every window's hf against 450: 8 Hz for mf, 32 Hz (amplitude x) for hf, period 16 samples
    n = 128 + 16 * 5
    return tone(MID, 8.0, 128.0, n) + tone(x, 32.0, 128.0, n), 128.0


TRIP = {"rank50": ("rank", 50.0, 0.05, 1.0), "mfmax50": ("mf", 50.0, 0.05, 1.0), "lf650": ("lf", 650.0, 0.5, 50.0), "hf450": ("hf", 450.0, 0.05, 50.0)}


@functools.lru_cache(maxsize=None)
def trip_pair(kind):
    key, trip, lo, hi = TRIP[kind]
    at = 0 if kind == "hf450" else 2

    def f(x):
        g, rate = trip_clip(kind, x)
        if kind == "hf450":
            g = g[:, :128]                                                           # every window holds the same samples: one is enough for the search
        return float(statement(g, rate, 1, ALL)[key][at])
    return straddle(f, lo, hi, trip)


# ---- preconditions (on the statement's dict s and the case c) ----------------------------------------------------------------------------------------------
def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def kept(s):
    return [int(i) for i in np.flatnonzero(~(s["rank_nms"] == 0.0))]                  # survivors of the suppression, NaN included


def windows_of_points(s, c):
    n = S.fft_size(c.rate)
    return [int(round((p / 1000.0 * c.rate - n / 2.0) / 16.0)) for p in s["points"]]


def pre_kept(want, points=None):
    def pre(s, c):
        assert kept(s) == sorted(want), (kept(s), want)
        if points is not None:
            assert windows_of_points(s, c) == list(points), (windows_of_points(s, c), points)
    return pre


def pre_masked(want):
    def pre(s, c):
        got = [int(i) for i in np.flatnonzero(s["masked"] != 0.0)]
        assert got == list(want), (got, want)
    return pre


def pre_points(want):
    def pre(s, c):
        assert windows_of_points(s, c) == list(want), (windows_of_points(s, c), want)
    return pre


def pre_equal(i, j):
    def pre(s, c):
        assert u32(s["rank"])[i] == u32(s["rank"])[j]
    return pre


def pre_all(*pres):
    def pre(s, c):
        for p in pres:
            p(s, c)
    return pre


def pre_plateau(lo, hi):
    """windows lo .. hi - 1 rank bit-equal above 50, and none of them is cleared"""
    def pre(s, c):
        r = u32(s["rank"][lo:hi])
        assert len(r) == hi - lo and np.all(r == r[0]) and s["rank"][lo] > 50.0
        assert np.array_equal(u32(s["rank_nms"][lo:hi]), u32(s["masked"][lo:hi]))
    return pre


def pre_nan(count, normal=True):
    def pre(s, c):
        assert int(np.count_nonzero(np.isnan(s["rank"]))) == count, int(np.count_nonzero(np.isnan(s["rank"])))
        assert int(np.count_nonzero(np.isnan(s["mf"]))) == count and s["low_motion"] == (not normal)
    return pre


def pre_formula(low_motion):
    """which formula was taken, told apart on a window where the two differ"""
    def pre(s, c):
        with np.errstate(all="ignore"):
            low = (s["lf"] + s["mf"]) / (F32(1.0) + S.nlfunc(s["hf"], F32(450.0)) * F32(0.003))
        assert s["low_motion"] == low_motion
        differ = ~S.same_bits_nan(low, s["rank"])
        assert differ != low_motion and np.any(s["lf"] > 0.0)
    return pre


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------
def _table():
    t = {}

    def add(name, group, branch, gyro, target=1, trims=ALL, rate=R16, broken_by=(), pre=None):
        assert name not in t and pre is not None, name
        g = gyro if gyro is None else _frozen(gyro)                                      # None: a trip-point case, filled in by case()
        t[name] = Case(group, branch, g, float(rate), int(target), tuple((float(a), float(b)) for a, b in trims), tuple(broken_by), pre)

    # ---- suppression window: the reference clears j in [i - r, i + r) and [0, len - 1) — not symmetric ----
    for rate, r in ((16.0, 4), (15.5, 3)):
        assert S.as_usize(rate / 16.0 / 2.0 * 8.0) == r and S.fft_size(rate) == 16 and S.band_bins(16, rate) == [0, 2, 7, 7]
        for d in (r - 1, r, r + 1):
            tag = "sup_r%d_" % r
            add(tag + "before_%d" % d, "suppression", "a lower neighbour %d before a peak (r = %d): %s" % (d, r, "cleared" if d <= r else "survives"),
                profile(20, {10: HIGH, 10 - d: LOW}), rate=rate, pre=pre_kept([10] + ([10 - d] if d > r else []), [10]))
            add(tag + "behind_%d" % d, "suppression", "a lower neighbour %d behind a peak (r = %d): %s" % (d, r, "cleared" if d < r else "survives"),
                profile(20, {10: HIGH, 10 + d: LOW}), rate=rate, pre=pre_kept([10] + ([10 + d] if d >= r else []), [10]),
                broken_by=["nms_symmetric"] if d == r else [])
    add("sup_plateau_8", "suppression", "8 equal ranks: `<` clears nothing", lay([MID] * 8), pre=pre_all(pre_plateau(0, 8), pre_kept(range(8), [7])),
        broken_by=["nms_le", "pick_first_across"])
    add("sup_plateau_20", "suppression", "20 equal ranks under the two-second rule: windows 2 .. 17 all survive", lay([MID] * 20),
        pre=pre_all(pre_plateau(2, 18), pre_kept(range(2, 18), [17])), broken_by=["nms_le"])
    add("sup_peak_last", "suppression", "the peak in the last window clears the four before it", lay([LOW] * 9 + [HIGH]), pre=pre_kept([0, 1, 2, 3, 4, 9], [9]))
    add("sup_peak_before_last", "suppression", "a higher peak just before the last window: the last element is never cleared", lay([0] * 8 + [HIGH, LOW]), target=10,
        pre=pre_kept([8, 9], [8, 9]), broken_by=["nms_last_cleared"])
    ladder = [TOP, HIGH, MID, LOW, 1.5]
    for n in (1, 2, 4, 5):
        add("sup_count_%d_down" % n, "suppression", "%d window(s), falling: the first clears what lies within r - 1 behind it, never the last" % n, lay(ladder[:n]),
            pre=pre_kept(sorted({0, n - 1}), [n - 1] if n == 1 else [0]), broken_by=["nms_last_cleared"] if n > 1 else [])
        add("sup_count_%d_up" % n, "suppression", "%d window(s), rising: every window but the last is cleared" % n, lay(ladder[:n][::-1]), pre=pre_kept([n - 1], [n - 1]))
    add("sup_tile_high_first", "suppression", "windows 255 and 256 straddle a 256-window tile of the nms kernel: the higher first", profile(300, {255: HIGH, 256: LOW}),
        pre=pre_kept([255], [255]))
    add("sup_tile_high_second", "suppression", "windows 255 and 256 straddle a 256-window tile: the higher second", profile(300, {255: LOW, 256: HIGH}),
        pre=pre_kept([256], [256]))

    # ---- pick: segments of 1, 256, 257, 512, 513, 600 windows — a lane's run is 1, 1, 2, 2, 3, 3 ----
    add("pick_segment_1", "pick", "a clip of one window, one segment", lay([HIGH]), pre=pre_kept([0], [0]))
    for n in (256, 257, 512, 513, 600):
        run = (n + 255) // 256
        add("pick_ends_%d" % n, "pick", "a segment of %d windows (a lane's run is %d): equal maxima in the first and the last lane that hold any, the last wins" % (n, run),
            profile(n, {2: HIGH, n - 3: HIGH}), pre=pre_all(pre_kept([2, n - 3], [n - 3]), pre_equal(2, n - 3)),
            broken_by=["pick_first_across"])
    add("pick_equal_in_run", "pick", "600 windows, lane 100 folds 300 .. 302: equal maxima at 300 and 301, the later wins", profile(600, {300: HIGH, 301: HIGH, 50: MID}),
        pre=pre_kept([50, 300, 301], [301]), broken_by=["pick_first_in_run"])
    add("pick_equal_in_run_of_2", "pick", "400 windows, lane 100 folds 200 and 201: equal maxima in both, the later wins", profile(400, {200: HIGH, 201: HIGH, 350: MID}),
        pre=pre_kept([200, 201, 350], [201]), broken_by=["pick_first_in_run"])
    add("pick_equal_neighbour_lanes", "pick", "600 windows: equal maxima at 302 (lane 100) and 303 (lane 101), the later wins", profile(600, {302: HIGH, 303: HIGH, 50: MID}),
        pre=pre_kept([50, 302, 303], [303]), broken_by=["pick_first_across"])
    add("pick_segment_border", "pick", "two segments of 300: equal maxima in the first one's last window and the second one's first", profile(600, {299: HIGH, 300: HIGH}),
        target=2, pre=pre_kept([299, 300], [299, 300]))
    add("pick_target_7", "pick", "7 does not divide 600: segments of 86, the last of 84; equal maxima in a segment's last window and the next one's first (257 | 258, 515 | 516), "
        "two equal ones in segment 3", profile(600, {5: MID, 171: LOW, 257: HIGH, 258: HIGH, 300: HIGH, 400: TOP, 515: LOW, 516: LOW, 597: HIGH}), target=7,
        pre=pre_kept([5, 171, 257, 258, 300, 400, 515, 516, 597], [5, 171, 257, 300, 400, 515, 597]), broken_by=["pick_first_across"])
    add("pick_short_last", "pick", "513 windows in two segments: 257 (a lane's run is 2) and 256 (the run is counted anew: 1)", profile(513, {100: MID, 256: HIGH, 257: HIGH, 400: MID, 401: MID}),
        target=2, pre=pre_kept([100, 256, 257, 400, 401], [256, 257]))
    add("pick_last_of_one", "pick", "601 windows, target 300: segments of 3, segment 200 is the last window alone (cleared by the two-second rule), 99 segments start beyond the end",
        profile(601, {3: MID, 4: MID, 5: MID, 300: HIGH, 597: LOW, 599: TOP, 600: TOP}), target=300, pre=pre_kept([3, 4, 5, 300, 597], [5, 300, 597]),
        broken_by=["pick_first_across"])
    add("pick_beyond_end", "pick", "10 windows, 14 segments of one window: four start beyond the end", lay([MID] * 10), target=14,
        pre=pre_all(pre_plateau(0, 10), pre_kept(range(10), range(10))), broken_by=["nms_le"])
    add("pick_zero_between", "pick", "three segments of 200, the middle one all zero", profile(600, {100: MID, 500: HIGH}), target=3, pre=pre_kept([100, 500], [100, 500]))

    # ---- gather: segments with and without a pick alternate in runs ----
    on = [(i % 23) < 9 or 300 <= i < 340 or i % 7 == 0 for i in range(600)]
    for i in range(600):
        on[i] = (on[i] or 256 <= i < 512) and not 100 <= i < 160                       # a whole lane of 256 segments with picks, 60 segments without any
    runs = lay([MID if v else 0 for v in on])
    for target in (1, 255, 256, 257, 600, TARGET_MAX):
        def pre(s, c, target=target):
            has = s["seg_pick"] >= 0
            assert len(has) == target and len(s["points"]) == int(np.count_nonzero(has)) and np.all(np.diff(s["points"]) > 0.0)
            run = (target + 255) // 256
            counts = {int(np.count_nonzero(has[l * run:(l + 1) * run])) for l in range(256) if l * run < target}
            if target >= 600:
                assert 0 in counts and run in counts and any(0 < v < run for v in counts), sorted(counts)          # a lane's count: none, its whole run, in between
            if target > 1:
                assert 0 < len(s["points"]) < target
        add("gather_%d" % target, "gather", "target %d over 600 windows: %d segment(s) a lane of the gather stage" % (target, (target + 255) // 256), runs, target=target, pre=pre,
            broken_by=["gather_interleaved"] if target in (600, TARGET_MAX) else [])

    # ---- times (rate 16.0: window i is at exactly i seconds) ----
    add("time_12_windows", "times", "total_duration == 12.0: the two-second rule is off", lay([MID] * 12), target=12, pre=pre_all(pre_masked(range(12)), pre_plateau(0, 12)),
        broken_by=["ge_12"])
    add("time_13_windows", "times", "13 windows: 0, 1, 11 and 12 are cleared, 2 and 10 kept", lay([MID] * 13), target=13, pre=pre_masked(range(2, 11)),
        broken_by=["time_le_2", "time_gt_total"])
    trims = {"point": ([(3.0, 3.0)], [3], "(3.0, 3.0) is exactly window 3"), "inclusive": ([(3.0, 5.0)], [3, 4, 5], "(3.0, 5.0) is inclusive at both ends"),
             "between": ([(3.25, 3.75)], [], "a range strictly between two window times covers nothing"), "inverted": ([(5.0, 4.0)], [], "an inverted range covers nothing"),
             "inf_both": ([(-INF, INF)], range(10), "(-inf, inf) covers everything"), "inf_low": ([(-INF, 3.0)], range(4), "(-inf, 3.0)"), "inf_high": ([(6.0, INF)], range(6, 10), "(6.0, inf)"),
             "nan": ([(NAN, 5.0), (0.0, NAN), (NAN, NAN)], [], "a NaN bound matches nothing"),
             "last_of_1024": ([(100.0 + i, 101.0 + i) for i in range(TRIM_MAX - 1)] + [(3.0, 5.0)], [3, 4, 5], "1024 ranges of which only the last matches"),
             "overlap": ([(2.0, 5.0), (4.0, 7.0)], range(2, 8), "two overlapping ranges")}
    for k, (tr, want, branch) in trims.items():
        add("time_trim_" + k, "times", "trim: " + branch, lay([MID] * 10), target=10, trims=tr, pre=pre_all(pre_masked(want), pre_points(want)),
            broken_by=["trim_exclusive"] if k in ("point", "inclusive") else [])

    # ---- trip points ----
    for kind in TRIP:
        key, trip, _, _ = TRIP[kind]
        for side in ("below", "above", "exact"):                                         # "exact" is kept aside: exact_names() lists it where the hit exists
            at = 0 if kind == "hf450" else 2

            def pre(s, c, kind=kind, key=key, trip=trip, side=side, at=at):
                v = float(s[key][at])
                assert (v < trip) == (side == "below") and (side != "exact" or v == trip), (kind, side, v)
                if kind == "rank50":
                    assert not s["low_motion"] and (s["masked"][2] == 0.0) == (side == "below")
                elif kind == "mfmax50":
                    assert float(s["mf"].max()) == v
                    pre_formula(side == "below")(s, c)                               # one window at or above 50 changes EVERY window's formula
                elif kind == "lf650":
                    assert not s["low_motion"] and s["mf"][2] >= 50.0
                else:
                    assert not s["low_motion"] and len(s["hf"]) == 6 and np.all(u32(s["hf"]) == u32(s["hf"])[0]) and S.band_bins(128, 128.0) == [0, 2, 30, 63]
            add("trip_%s_%s" % (kind, side), "trips", "%s %s %g at an amplitude found on the statement" % (key, {"below": "<", "above": ">=", "exact": "=="}[side], trip),
                None, rate=128.0 if kind == "hf450" else R16, target=2, pre=pre)

    # ---- non-finite and extreme samples ----
    nan_block = poked(tone(MID), 1, 5, NAN)
    for where, w in (("first", 300), ("inside", 301), ("last", 302)):
        add("nan_run_" + where, "nonfinite", "one NaN sample in window %d, %s in lane 100's run of 300 .. 302, peaks before and behind" % (w, where),
            profile(600, {100: HIGH, w: nan_block, 450: MID}), pre=pre_all(pre_nan(1), pre_kept([100, w, 450], [450])),
            broken_by=["no_nan_reset"] if where != "last" else [])
    add("nan_repro", "nonfinite", "the pick under NaN: a plateau with its maximum in window 30 and one NaN sample in window 34, the middle of lane 11's run — the fold restarts behind it",
        profile(600, {30: TOP, 34: nan_block}, fill=MID), pre=pre_all(pre_nan(1), pre_points([597])), broken_by=["no_nan_reset"])
    add("nan_repro_run_end", "nonfinite", "the twin with the NaN in window 35, the end of lane 11's run", profile(600, {30: TOP, 35: nan_block}, fill=MID),
        pre=pre_all(pre_nan(1), pre_points([597])))
    add("nan_repro_larger_behind", "nonfinite", "the twin with a larger value behind the NaN", profile(600, {30: TOP, 34: nan_block, 100: 8.0}, fill=MID),
        pre=pre_all(pre_nan(1), pre_points([100])))
    add("nan_segment_end", "nonfinite", "a NaN in the last window of segment 0 of 3: the pick IS the NaN window and a point is emitted (`NaN < 0.1` is false)",
        profile(600, {199: nan_block}, fill=MID), target=3, pre=pre_all(pre_nan(1), pre_points([199, 399, 597])))
    add("nan_segment_all", "nonfinite", "segment 1 of 3 is all NaN", profile(600, {i: nan_block for i in range(200, 400)}, fill=MID), target=3,
        pre=pre_all(pre_nan(200), pre_points([199, 399, 597])))
    add("nan_beside_peak", "nonfinite", "a NaN window next to a peak: it is neither cleared nor does it clear; mf_max ignores its NaN and the normal formula is taken",
        profile(12, {3: LOW, 4: nan_block, 5: HIGH, 6: LOW, 9: LOW}), target=12, pre=pre_all(pre_nan(1), pre_kept([4, 5, 9], [4, 5, 9])))
    add("nan_low_motion", "nonfinite", "an mf that holds a NaN while every other mf < 50: the fold ignores the NaN and the LOW-motion formula is taken",
        profile(10, {2: 0.2, 5: poked(dc(1.5, 0.1), 0, 7, NAN), 8: dc(1.0, 0.05)}), target=2, pre=pre_all(pre_nan(1, normal=False), pre_formula(True)), broken_by=["max_propagating"])

    def pre_nonfinite(s, c):
        assert np.all(np.isfinite(s["rank"][[0, 1, 3, 4, 5]])) and not np.isfinite(s["rank"][2]) and s["rank"][4] > 50.0
    for name, axis, sample, v, branch in (("pinf", 0, 5, INF, "+inf at sample 5 of one axis: inf and NaN meet in the folds and under the root"), ("ninf", 2, 0, -INF, "-inf at sample 0: s[0] = 0.0, so every bin's imaginary part is a NaN from its first term"),
                                          ("1e300", 1, 9, 1e300, "1e300 is `as f32` inf through the staging"), ("3e38", 1, 9, 3e38, "3e38 is finite in f32; the fold overflows")):
        def pre(s, c, name=name):
            pre_nonfinite(s, c)
            with np.errstate(all="ignore"):
                assert np.isfinite(c.gyro.astype(F32)).all() == (name == "3e38")
        add("extreme_" + name, "nonfinite", branch, profile(6, {2: poked(poked(poked(tone(MID), 0, 9, 2.5e38), 2, 9, 2.9e38) if name == "3e38" else tone(MID), axis, sample, v), 4: HIGH}), target=6, pre=pre)

    def pre_tiny(zero):
        def pre(s, c):
            assert s["low_motion"] and np.all(s["masked"] == 0.0) and len(s["points"]) == 0
            e = np.concatenate([s["lf"], s["mf"]])
            if zero:                                                                 # the squares underflow in IEEE arithmetic too: exactly +0.0, whatever the build does with subnormals
                assert np.all(u32(e) == 0)
            else:                                                                    # the squares are subnormal f32 and the roots normal: flush-to-zero would give 0
                assert np.all(s["mf"] > 0.0) and len(set(u32(s["mf"]).tolist())) == len(s["mf"])
                assert np.all((s["mf"].astype(np.float64) / 4.0) ** 2 < 2.0 ** -126)         # a magnitude under the root is at most mf / scale, scale = 4 at N = 16
        return pre
    add("tiny_subnormal_samples", "nonfinite", "windows of subnormal amplitude (1e-40, 1e-41, 1e-42) and of -0.0: subnormal products and sums, squares that underflow to +0.0",
        lay([tone(1e-40), tone(1e-41), tone(1e-42), -ZERO, dc(1e-41)]), target=5, pre=pre_tiny(True))
    add("tiny_subnormal_squares", "nonfinite", "amplitudes 1e-21 .. 5e-23: the squares under the root are subnormal, the band energies are not — equal to the statement's only without flush-to-zero",
        lay([tone(1e-21), tone(5e-22), tone(2e-22), tone(1e-22), tone(5e-23)]), target=5, pre=pre_tiny(False))
    return t


def _frozen(gyro):
    g = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1))
    g.setflags(write=False)
    return g


_SPECS = _table()                                                                    # name -> Case; gyro is None where the samples wait for the statement
NAMES = sorted(n for n in _SPECS if not n.endswith("_exact"))
GROUPS = sorted({c.group for c in _SPECS.values()})


@functools.lru_cache(maxsize=None)
def exact_names():
    """the trip-point cases whose amplitude hits the constant exactly: they exist where the search found such a hit"""
    return tuple("trip_%s_exact" % kind for kind in TRIP if trip_pair(kind)[2])


def all_names():
    return NAMES + list(exact_names())


@functools.lru_cache(maxsize=None)
def case(name):
    c = _SPECS[name]
    if c.gyro is None:
        _, kind, side = name.split("_")
        a, b, exact = trip_pair(kind)
        assert side != "exact" or exact, name
        g, rate = trip_clip(kind, a if side == "below" else b)
        assert rate == c.rate
        c = c._replace(gyro=_frozen(g))
    return c


KEYS = ("lf", "mf", "hf", "rank", "masked", "rank_nms", "points")
REPRO = "nan_repro"
DEVICE_OUTPUT_CASES = ("nan_repro", "nan_segment_all", "nan_beside_peak", "gather_600")     # also run with device outputs on the GPU tier
MIRROR_CASE = "nan_segment_end"                                                             # OptimSync.run on the GPU tier


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    s = statement(c.gyro, c.rate, c.target, c.trims)
    c.pre(s, c)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def compare(name, got, keys=KEYS):
    """every output named in `keys` against the statement under the rule for this table: NaNs at the same indices with any sign or payload, everything else equal as
    uint32 / uint64 views.  -> the keys that differ (the caller asserts there are none, so that a failure names them all)"""
    s = reference(name)
    return [k for k in keys if not S.same_bits_nan(np.asarray(got[k]), s[k])]
