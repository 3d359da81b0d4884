"""The case table of tests/_optimcase.py held to account before any kernel sees it (no GPU): every case's precondition on the f32 statement; the statement's tail
(tests/_syncoptimstmt.tail, total now: `mf_max` is the NaN-ignoring fold from 0.0) against the reference's own loops, transliterated and started from the statement's
band energies (tests/test_sync_optim_statement.reference_from_bands); a restatement of the DEVICE's algorithm — lanes folding strided and contiguous runs, lane 0
folding the lanes, a prefix sum for the gather — against both, and fourteen wrong variants of that restatement, each of which must change the cases that name it;
and tools/sync_optim_loop.cpp over the whole table.

Comparison rule for this table (S.same_bits_nan): NaNs at the same indices, with any sign or payload; everything else equal as uint32 / uint64 views."""
import numpy as np
import pytest

import _optimcase as O
import _syncoptimstmt as S
from test_sync_optim_statement import f32_max, reference_from_bands
from test_sync_optim_loop import loop

F32 = np.float32
LANES = 256
VARIANTS = ("nms_le", "nms_symmetric", "nms_last_cleared", "pick_first_in_run", "pick_first_across", "no_nan_reset", "trim_exclusive", "ge_12", "time_le_2",
            "time_gt_total", "le_50", "max_propagating", "le_01", "gather_interleaved")

# Band energies written down rather than computed from samples, for the two constants no amplitude is promised to hit exactly: (lf, mf, hf, rate, target)
TABULATED = {
    "mf_max_exactly_50": ([100.0, 700.0, 5.0, 0.0], [10.0, 50.0, 30.0, 49.0], [0.0, 500.0, 0.0, 0.0], 16.0, 2),        # 50 is not < 50: the normal formula
    "mf_max_below_50": ([100.0, 700.0, 5.0, 0.0], [10.0, 49.999996, 30.0, 49.0], [0.0, 500.0, 0.0, 0.0], 16.0, 2),
    "rank_exactly_50": ([0.0] * 6, [50.0, 0.0, 200.0, 0.0, 49.999996, 50.000004], [0.0] * 6, 16.0, 6),                  # 50 is not < 50: kept
    "mf_max_with_nan": ([10.0, 20.0, 30.0], [60.0, float("nan"), 40.0], [0.0] * 3, 16.0, 3),
    "mf_all_nan": ([10.0, 20.0], [float("nan"), float("nan")], [0.0] * 2, 16.0, 2),                                      # the fold stays 0.0: low motion
}


# ---- the device's algorithm, restated (gfw_sync_optim.hip behind the spectrum stage) --------------------------------------------------------------------------
def device_tail(lf, mf, hf, rate, n, target, trims, wrong=None):
    """-> dict(rank, masked, rank_nms, points, low_motion).  `wrong`: one of VARIANTS, switched here and nowhere else"""
    T = F32
    lf, mf, hf = (np.asarray(a, dtype=T) for a in (lf, mf, hf))
    w = len(mf)

    def fmax(a, b):
        if wrong == "max_propagating" and (a != a or b != b):
            return T(np.nan)
        return f32_max(a, b)
    # max kernel: lane t folds mf[t], mf[t + 256], ..; lane 0 folds the lanes
    lanes = []
    for t in range(LANES):
        m = T(0.0)
        for i in range(t, w, LANES):
            m = fmax(m, mf[i])
        lanes.append(m)
    mf_max = lanes[0]
    for j in range(1, LANES):
        mf_max = fmax(mf_max, lanes[j])
    low_motion = bool(mf_max <= T(50.0)) if wrong == "le_50" else bool(mf_max < T(50.0))
    # rank kernel: a lane is a window
    with np.errstate(all="ignore"):
        if low_motion:
            rank = (lf + mf) / (T(1.0) + S.nlfunc(hf, T(450.0)) * T(0.003))
        else:
            rank = mf / (T(1.0) + S.nlfunc(hf, T(450.0)) * T(0.003)) / (T(1.0) + S.nlfunc(lf, T(650.0)) * T(0.003))
        rank = rank.astype(T)
        ratio = 16.0 / float(rate)
        time = np.arange(w, dtype=np.float64) * ratio
        inside = np.zeros(w, dtype=bool)
        for a, b in np.asarray(trims, dtype=np.float64).reshape(-1, 2):
            inside |= ((time > a) & (time < b)) if wrong == "trim_exclusive" else ((time >= a) & (time <= b))
        low = (rank <= T(50.0)) if wrong == "le_50" else (rank < T(50.0))
        masked = np.where(low | ~inside, T(0.0), rank).astype(T)
        total = w * ratio
        if (total >= 12.0) if wrong == "ge_12" else (total > 12.0):
            head = (time <= 2.0) if wrong == "time_le_2" else (time < 2.0)
            foot = (time > (total - 2.0)) if wrong == "time_gt_total" else (time >= (total - 2.0))
            masked[head | foot] = T(0.0)
        # nms kernel: element j looks at i in (j - r, j + r], clamped to 0 .. len - 1; the last element is left alone
        r = S.as_usize(float(rate) / 16.0 / 2.0 * 8.0)
        j = np.arange(w)
        clear = np.zeros(w, dtype=bool)
        for d in range(-r if wrong == "nms_symmetric" else -r + 1, r + 1):
            i = j + d
            ok = (i >= 0) & (i <= w - 1)
            other = masked[np.clip(i, 0, max(w - 1, 0))]
            clear |= ok & ((masked <= other) if wrong == "nms_le" else (masked < other))
        if w and wrong != "nms_last_cleared":
            clear[w - 1] = False
        rank_nms = np.where(clear, T(0.0), masked).astype(T)
    # pick kernel: a workgroup is a segment, a lane folds a contiguous run, lane 0 the lanes in order
    seg = (w + target - 1) // target
    seg_ms = np.full(target, -1.0)
    for s in range(target):
        start = s * seg
        cnt = max(min(start + seg, w) - start, 0)
        run = (cnt + LANES - 1) // LANES
        per_lane = []
        for t in range(LANES if run else 0):
            c0, c1 = min(t * run, cnt), min(t * run + run, cnt)
            if c0 == c1:
                break                                                                # this lane and every later one hold nothing
            best, idx, reset = T(0.0), -1, False
            for c in range(c0, c1):
                v = rank_nms[start + c]
                if idx < 0 or ((v > best) if wrong == "pick_first_in_run" else not (best > v)):
                    best, idx = v, c
                reset = reset or bool(v != v)
            per_lane.append((best, idx, reset and wrong != "no_nan_reset"))
        pick, high = -1, T(0.0)
        for best, idx, reset in per_lane:
            if pick < 0 or reset or ((best > high) if wrong == "pick_first_across" else not (high > best)):
                high, pick = best, idx
        if pick >= 0 and not ((high <= T(0.1)) if wrong == "le_01" else (high < T(0.1))):
            seg_ms[s] = (float(start + pick) * 16.0 + float(n) / 2.0) / float(rate) * 1000.0
    # gather kernel: a lane owns a contiguous run of segments; lane 0 turns the counts into offsets
    run = (target + LANES - 1) // LANES
    own = [list(range(t, target, LANES)) if wrong == "gather_interleaved" else list(range(min(t * run, target), min(t * run + run, target))) for t in range(LANES)]
    counts = [sum(1 for c in o if seg_ms[c] >= 0.0) for o in own]
    points = np.full(sum(counts), -7.0)
    at = 0
    for t in range(LANES):
        k = at
        for c in own[t]:
            if seg_ms[c] >= 0.0:
                points[k] = seg_ms[c]
                k += 1
        at += counts[t]
    return dict(rank=rank, masked=masked, rank_nms=rank_nms, points=points, low_motion=low_motion)


def differs(a, b):
    return [k for k in ("rank", "masked", "rank_nms", "points") if not S.same_bits_nan(a[k], b[k])] + ([] if a["low_motion"] == b["low_motion"] else ["low_motion"])


_device = {}


def device(name, wrong=None):
    if (name, wrong) not in _device:
        c, s = O.case(name), O.reference(name)
        _device[name, wrong] = device_tail(s["lf"], s["mf"], s["hf"], c.rate, S.fft_size(c.rate), c.target, c.trims, wrong)
    return _device[name, wrong]


def tabulated(name, wrong=None):
    lf, mf, hf, rate, target = TABULATED[name]
    a = [np.array(v, dtype=F32) for v in (lf, mf, hf)]
    with np.errstate(all="ignore"):
        return S.tail(*a, rate, 16, target, O.ALL, F32), reference_from_bands(*a, rate, 16, target, list(O.ALL)), device_tail(*a, rate, 16, target, O.ALL, wrong)


# ---- the table itself ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_names_every_branch_of_the_issue_and_its_limits_are_the_librarys():
    from gyroflow_amd import abi
    assert (O.TARGET_MAX, O.TRIM_MAX) == (abi.SYNC_OPTIM_TARGET_MAX, abi.SYNC_OPTIM_TRIM_MAX)
    assert O.GROUPS == ["gather", "nonfinite", "pick", "suppression", "times", "trips"] and len(O.NAMES) >= 80
    assert all(v in VARIANTS for n in O.NAMES for v in O.case(n).broken_by)
    for c in (O.case(n) for n in O.all_names()):
        w = S.n_windows(c.gyro.shape[1], S.fft_size(c.rate))
        assert 1 <= w <= 800 and (c.rate == 128.0 or (S.fft_size(c.rate) == 16 and c.gyro.shape[1] == 16 * w))        # disjoint windows of 16 samples
    for kind in O.TRIP:
        a, b, exact = O.trip_pair(kind)
        assert np.nextafter(F32(a), F32(np.inf)) == F32(b)                               # neighbouring f32 amplitudes
        assert ("trip_%s_exact" % kind in O.exact_names()) == exact


@pytest.mark.parametrize("name", O.NAMES)
def test_the_precondition_holds_on_the_statement(name):
    s = O.reference(name)                                                                # asserts the case's precondition
    c = O.case(name)
    assert len(s["rank"]) == S.n_windows(c.gyro.shape[1], S.fft_size(c.rate)) and not any(v.flags.writeable for v in s.values() if isinstance(v, np.ndarray))


@pytest.mark.parametrize("name", O.NAMES)
def test_the_tail_equals_the_reference_loops_from_the_statements_band_energies(name):
    c, s = O.case(name), O.reference(name)
    pts, rank, masked, nms, low = reference_from_bands(s["lf"], s["mf"], s["hf"], c.rate, S.fft_size(c.rate), c.target, list(c.trims))
    assert low == s["low_motion"]
    assert S.same_bits_nan(rank, s["rank"]) and S.same_bits_nan(masked, s["masked"]) and S.same_bits_nan(nms, s["rank_nms"])
    assert S.same_bits_nan(pts, s["points"]), (pts, s["points"])


@pytest.mark.parametrize("name", O.NAMES)
def test_the_devices_algorithm_restated_equals_the_statement(name):
    assert differs(device(name), O.reference(name)) == []


@pytest.mark.parametrize("name", sorted(TABULATED))
def test_tabulated_band_energies_at_the_constants(name):
    tail, (pts, rank, masked, nms, low), dev = tabulated(name)
    assert low == tail["low_motion"] == {"mf_max_exactly_50": False, "mf_max_below_50": True, "rank_exactly_50": False, "mf_max_with_nan": False, "mf_all_nan": True}[name]
    assert S.same_bits_nan(rank, tail["rank"]) and S.same_bits_nan(masked, tail["masked"]) and S.same_bits_nan(nms, tail["rank_nms"]) and S.same_bits_nan(pts, tail["points"])
    assert differs(dev, tail) == []
    if name == "rank_exactly_50":
        assert list(tail["masked"] != 0.0) == [True, False, True, False, False, True]


def test_the_comparison_rule():
    nan, other = np.array([np.nan], dtype=F32), np.array([0xFFC00123], dtype=np.uint32).view(F32)
    a = np.array([1.0, nan[0], -0.0], dtype=F32)
    b = np.array([1.0, other[0], -0.0], dtype=F32)
    assert not S.same_bits(a, b) and S.same_bits_nan(a, b)                                # a NaN of another sign and payload
    assert not S.same_bits_nan(a, np.array([1.0, nan[0], 0.0], dtype=F32))                # -0.0 is not 0.0
    assert not S.same_bits_nan(a, np.array([nan[0], 1.0, -0.0], dtype=F32)) and not S.same_bits_nan(a, a.astype(np.float64)) and not S.same_bits_nan(a, a[:2])
    assert S.same_bits_nan(np.zeros(0), np.zeros(0))


# ---- wrong variants --------------------------------------------------------------------------------------------------------------------------------------------
# What each variant changes: the cases of the table (every one that names the variant in `broken_by` must be among them) and the tabulated band energies above.
# `le_01` changes nothing, and cannot: a masked rank is 0.0, at least 50.0 or a NaN, so no value that reaches `< 0.1` lies near 0.1 — the compare is exercised at
# 0.0 (no point) and at NaN (a point) only.  `le_50` needs a rank or an mf_max of exactly 50.0, which no amplitude is promised to give: the tabulated energies do.
# Every case of the table (by name: the exact hits aside) that a variant changes, as found when the table was written; asserted as it stands.
CHANGES = {
    "nms_le": (
        "extreme_1e300 extreme_3e38 extreme_ninf extreme_pinf gather_1 gather_255 gather_256 gather_257 gather_600 gather_65535 nan_beside_peak nan_low_motion "
        "nan_repro nan_repro_larger_behind nan_repro_run_end nan_run_first nan_run_inside nan_run_last nan_segment_all nan_segment_end pick_beyond_end "
        "pick_ends_256 pick_ends_257 pick_ends_512 pick_ends_513 pick_ends_600 pick_equal_in_run pick_equal_in_run_of_2 pick_equal_neighbour_lanes "
        "pick_last_of_one pick_segment_border pick_short_last pick_target_7 pick_zero_between sup_count_2_down sup_count_4_down sup_count_5_down "
        "sup_peak_before_last sup_peak_last sup_plateau_20 sup_plateau_8 sup_r3_before_2 sup_r3_before_3 sup_r3_before_4 sup_r3_behind_2 sup_r3_behind_3 "
        "sup_r3_behind_4 sup_r4_before_3 sup_r4_before_4 sup_r4_before_5 sup_r4_behind_3 sup_r4_behind_4 sup_r4_behind_5 sup_tile_high_first "
        "sup_tile_high_second time_12_windows time_13_windows time_trim_inclusive time_trim_inf_both time_trim_inf_high time_trim_inf_low "
        "time_trim_last_of_1024 time_trim_overlap time_trim_point trip_hf450_above trip_hf450_below trip_lf650_above trip_lf650_below trip_mfmax50_above "
        "trip_mfmax50_below trip_rank50_above trip_rank50_below "
    ).split(),
    "nms_symmetric": (
        "nan_beside_peak nan_repro_larger_behind nan_repro_run_end sup_r3_behind_3 sup_r4_behind_4 "
    ).split(),
    "nms_last_cleared": (
        "sup_count_2_down sup_count_4_down sup_count_5_down sup_peak_before_last "
    ).split(),
    "pick_first_in_run": (
        "pick_equal_in_run pick_equal_in_run_of_2 "
    ).split(),
    "pick_first_across": (
        "gather_1 gather_255 gather_256 gather_257 nan_low_motion nan_repro nan_repro_run_end nan_run_last nan_segment_all nan_segment_end pick_ends_256 "
        "pick_ends_257 pick_ends_512 pick_ends_513 pick_ends_600 pick_equal_neighbour_lanes pick_last_of_one pick_target_7 sup_plateau_20 sup_plateau_8 "
        "trip_hf450_above trip_hf450_below "
    ).split(),
    "no_nan_reset": (
        "nan_repro nan_run_first nan_run_inside "
    ).split(),
    "trim_exclusive": (
        "pick_beyond_end pick_segment_1 sup_count_1_down sup_count_1_up sup_count_2_down sup_count_2_up sup_count_4_down sup_count_4_up sup_count_5_down "
        "sup_count_5_up sup_peak_last sup_plateau_8 time_12_windows time_trim_inclusive time_trim_inf_high time_trim_inf_low time_trim_last_of_1024 "
        "time_trim_overlap time_trim_point trip_hf450_above trip_hf450_below "
    ).split(),
    "ge_12": (
        "time_12_windows "
    ).split(),
    "time_le_2": (
        "gather_1 gather_255 gather_256 gather_257 gather_600 gather_65535 nan_repro nan_repro_larger_behind nan_repro_run_end nan_segment_all nan_segment_end "
        "pick_ends_256 pick_ends_257 pick_ends_512 pick_ends_513 pick_ends_600 sup_plateau_20 time_13_windows "
    ).split(),
    "time_gt_total": (
        "gather_1 gather_255 gather_256 gather_257 gather_600 gather_65535 nan_repro nan_repro_larger_behind nan_repro_run_end nan_segment_all nan_segment_end "
        "pick_last_of_one sup_plateau_20 time_13_windows "
    ).split(),
    "le_50": (
        " "
    ).split(),
    "max_propagating": (
        "nan_low_motion "
    ).split(),
    "le_01": (
        " "
    ).split(),
    "gather_interleaved": (
        "gather_600 gather_65535 "
    ).split(),
}
CHANGED_TABULATED = {"le_50": ["mf_max_exactly_50", "rank_exactly_50"], "max_propagating": ["mf_all_nan"]}                # (with another mf >= 50 a propagated NaN is `not < 50` as well: the normal formula either way)


@pytest.mark.parametrize("wrong", VARIANTS)
def test_a_wrong_variant_changes_the_cases_that_name_it(wrong):
    named = sorted(n for n in O.NAMES if wrong in O.case(n).broken_by)
    changed = sorted(n for n in O.all_names() if differs(device(n, wrong), O.reference(n)))
    tab = sorted(n for n in TABULATED if differs(tabulated(n, wrong)[2], tabulated(n)[0]))
    print("%s changes %d cases: %s; tabulated: %s" % (wrong, len(changed), " ".join(changed), " ".join(tab)))
    assert set(named) <= set(changed), sorted(set(named) - set(changed))
    assert [n for n in changed if n in O.NAMES] == CHANGES[wrong]
    assert set(CHANGED_TABULATED.get(wrong, [])) <= set(tab), tab
    if wrong == "le_01":
        assert changed == [] and named == []
    elif wrong != "le_50":
        assert len(named) >= 1
    if wrong == "no_nan_reset":                                                          # the pick kernel before its fix: a NaN inside a lane's run, not at its end
        assert O.REPRO in changed and "nan_repro_run_end" not in changed and "nan_repro_larger_behind" not in changed and "nan_run_last" not in changed


# ---- tools/sync_optim_loop.cpp over the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.NAMES)
def test_the_cpp_loop_equals_the_statement(name):
    c = O.case(name)
    got = loop(c.gyro, c.rate, c.target, c.trims)
    assert O.compare(name, got, keys=("lf", "mf", "hf", "rank", "rank_nms", "points")) == []


def test_the_exact_hits_on_the_constants_where_the_search_found_one():
    """a trip-point amplitude whose statement value IS the constant, as a third case: through everything the other cases go through"""
    print("exact hits:", " ".join(O.exact_names()) or "none")
    for name in O.exact_names():
        test_the_precondition_holds_on_the_statement(name)
        test_the_tail_equals_the_reference_loops_from_the_statements_band_energies(name)
        test_the_devices_algorithm_restated_equals_the_statement(name)
        test_the_cpp_loop_equals_the_statement(name)
