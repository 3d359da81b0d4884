"""The case table of tests/_tablecase.py held to account before a kernel tier uses it (no device):

(a) the identity: for every case the statements' mapped points ARE the points handed in (uint32 views, NaN as NaN), and each case's precondition holds — k, the
    rejected rows per kind, the shares and n_valid of the compaction pairs, the distances at and above 2^31, the equal minima and their lanes, the exits and first
    indices of the zoom rounds, no lookup between unequal keys;
(b) the public-entry route through the interpreted kernels gives what the test-only table entries of the drivers (E.sync_table, E.zoom_table) give for the cases
    both can express;
(c) discrimination: a restatement of the device's algorithm here (bisection over counts, two-level reduce, the round loop) equals the statement on every case, and
    each wrong variant of it changes the result of the cases it names.  The variants are switched in this module only; the product knows none of them."""
import numpy as np
import pytest

import _emu_sync as ES
import _emu_zoom as EZ
import _syncstmt as SS
import _tablecase as T
import _zoomstmt as Z

f32 = np.float32
COSTS = {c.name: c for c in T.sync_cost_cases()}
SEARCHES = {c.name: c for c in T.search_cases()}
GROUPS = {g.name: g for g in T.zoom_groups()}


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(COSTS))
def test_cost_case_maps_onto_itself_and_reaches_its_branch(name):
    case = COSTS[name]
    costs = T.precondition_sync(case)
    w, h = case.clip.size
    for c in range(len(case.candidates)):
        assert costs[c] == float(sum(SS.fold(m[:, 0], m[:, 1], w, h) for m in case.table_of_pairs(c)))


def test_the_cost_table_holds_what_the_issue_lists():
    names = set(COSTS)
    for nv in T.K_OF:
        assert any(n.startswith("count-%d+" % nv) for n in names)
    hit = {nv for c in COSTS.values() for nv in c.more.get("n_valid", []) if c.name.startswith("compact")}
    assert {64, 65, 128} <= hit
    assert sum(c.rejects["lens-none"] for c in COSTS.values()) >= 4 and all(sum(c.rejects[k] for c in COSTS.values()) >= 10 for k in T.KINDS[:4])
    big = COSTS["largest-pair-two-values"]
    assert [len(p) for _, _, p, _ in big.pairs] == [3, 4096, 0, 130]
    assert len(COSTS["rolling-plateaus"].candidates) == 5


@pytest.mark.parametrize("name", list(SEARCHES))
def test_search_case_has_its_equal_minima_on_exact_plateaus(name):
    st = T.precondition_search(SEARCHES[name])
    assert len(st["fine"]) == 200


@pytest.mark.parametrize("name", list(GROUPS))
def test_zoom_group_takes_its_exits(name):
    st = T.precondition_zoom(GROUPS[name])
    assert len(st["fov"]) == len(GROUPS[name].frames)


def test_the_zoom_table_takes_every_exit_and_both_end_indices():
    exits, firsts = T.precondition_zoom_table(list(GROUPS.values()))
    print(exits, sorted(firsts))


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------
def emu_costs(case, mapped=True):
    return ES.sync_visual_costs(case.range.kp, case.clip.model, case.clip.digital, case.search(), case.pairs, case.candidates, case.clip.tracks, mapped=mapped)


@pytest.mark.parametrize("name", [n for n in COSTS if not n.startswith("largest")])
def test_public_cost_route_equals_the_table_route(name):
    case = COSTS[name]
    T.precondition_sync(case)
    first = np.concatenate([[0], np.cumsum([len(p) for _, _, p, _ in case.pairs])]).astype(np.int32)
    table, _, _ = ES.sync_table(case.expected, first, case.clip.size[0], case.clip.size[1])
    assert T.same_bits(emu_costs(case, mapped=False), table), name


def test_public_search_route_equals_the_table_route():
    case = SEARCHES["ties-600"]
    st = T.precondition_search(case)
    mapped = np.array([SS.mapped_points(case.range, o, r) for o, r in st["coarse"]], dtype=np.float32)
    first = np.concatenate([[0], np.cumsum([len(p) for _, _, p, _ in case.pairs])]).astype(np.int32)
    costs, res, fine = ES.sync_table(mapped, first, T.W, T.HT, st["coarse"], 0)
    a = case.args
    pub, pub_costs, _ = ES.sync_visual_search(case.range.kp, case.clip.model, case.clip.digital, case.search(), case.pairs, 0, case.clip.tracks, a["initial_offset"],
                                              a["search_size"], a["readout"], a["fps"])
    assert T.same_bits(costs, pub_costs) and (res.found, res.n_coarse, res.coarse_value, res.coarse_cost) == (pub.found, pub.n_coarse, pub.coarse_value, pub.coarse_cost)
    assert [tuple(r) for r in fine] == st["fine"]


@pytest.mark.parametrize("name", list(GROUPS))
def test_public_zoom_route_equals_the_table_route(name):
    group = GROUPS[name]
    st = T.precondition_zoom(group)
    kp, search, frames, rot = group.inputs()
    pub, _ = EZ.zoom_fovs(kp, group.clip.model, group.clip.digital, search, frames, rotations=rot)
    n = 0
    for k, f in enumerate(group.frames):
        if tuple(f["center"]) != (0.0, 0.0):
            continue                                                                # (the table entry has no zoom centre)
        seen = st["polygons"][k]
        refined = np.array(seen.get(1, [(0.0, 0.0)] * 63), dtype=np.float32)
        got = EZ.zoom_table(np.array(seen[0], dtype=np.float32), np.stack([refined] * 4), group.clip.size[0], group.clip.size[1], group.clip.out, group.clip.margin)
        assert T.same_bits(np.array([got]), pub[k:k + 1]), (name, f["name"], got, pub[k])
        n += 1
    assert n >= 5


# ---- (c) the device's algorithm restated, and its wrong variants ---------------------------------------------------------------------------------------
def model_fold(m, w, h, variant=None):
    """gfw_sync_fold over one pair's mapped points [n][2][2]: the bounds test, compaction in point order, the bisection for the k-th smallest over counts,
    sum(d < T) + (k - count(d < T)) * T -> int"""
    m = np.asarray(m, dtype=np.float32).reshape(-1, 2, 2)
    wf, hf = f32(w), f32(h)
    with np.errstate(all="ignore"):
        x, y = m[:, :, 0], m[:, :, 1]
        ok = ((x >= 0) & (x <= wf) & (y >= 0) & (y <= hf)).all(axis=1) if variant == "bounds-inclusive" else ((x > 0) & (x < wf) & (y > 0) & (y < hf)).all(axis=1)
        a, b = m[ok, 0], m[ok, 1]
        dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        d = ((dx * dx) + (dy * dy)).astype(np.uint32).astype(np.int64)
    n = len(d)
    k = int(np.floor(float(n) * 0.9 + 0.5)) if variant == "k-rounded" else int(float(n) * 0.9)
    if k <= 0:
        return 0
    key = (lambda v: np.asarray(v, dtype=np.uint32).astype(np.int32).astype(np.int64)) if variant == "signed-compare" else (lambda v: np.asarray(v, dtype=np.int64))
    with np.errstate(all="ignore"):
        bound = f32(f32(f32(f32(wf * wf) + f32(hf * hf)) * f32(1.001)) + f32(1.0))
    lo, hi = 0, int(bound) if bound < f32(4294967040.0) else 0xFFFFFFFF
    while lo < hi:
        mid = lo + (hi - lo) // 2
        cnt = int((key(d) < key(mid)).sum()) if variant == "count-strict" else int((key(d) <= key(mid)).sum())
        if cnt >= k:
            hi = mid
        else:
            lo = mid + 1
    below = key(d) < key(lo)
    total = int(d[below].sum())
    return total if variant == "no-remainder" else total + (k - int(below.sum())) * lo


def model_cost(case, c, variant=None):
    w, h = case.clip.size
    return float(sum(model_fold(m, w, h, variant) for m in case.table_of_pairs(c)))


def model_pick(costs, variant=None):
    """gfw_sync_reduce_kernel: 256 lanes stride over the candidates keeping their last minimum, lane 0 folds the lanes"""
    lanes = {}
    for i, c in enumerate(costs):
        t = i % 256
        if t not in lanes or (c < lanes[t][0] if variant == "first-minimum" else c <= lanes[t][0]):
            lanes[t] = (c, i)
    pick = None
    for t in sorted(lanes):
        c, i = lanes[t]
        if variant == "first-minimum":
            better = pick is None or c < pick[0] or (c == pick[0] and i < pick[1])
        elif variant == "no-cross-lane-tie-break":
            better = pick is None or c <= pick[0]                                   # the last minimum of the highest lane
        else:
            better = pick is None or c < pick[0] or (c == pick[0] and i > pick[1])
        if better:
            pick = (c, i)
    return pick[1]


def model_find_fov(group, frame, variant=None):
    """gfw_zoom_rounds over the statement's own map: the loop of fov_iterative.rs:91-134 as the kernel restates it -> fov f64"""
    clip = group.clip
    w, h = f32(clip.size[0]), f32(clip.size[1])
    mapper = Z.mapper_for(clip, 0, rotation=np.array(frame["rot"], dtype=np.float32))
    ratio = f32(w / f32(clip.out[0]))
    out0, out1 = f32(f32(clip.out[0]) * ratio), f32(f32(clip.out[1]) * ratio)
    inv_aspect = f32(out1 / out0)
    rect = Z.points_around_rect(w, h, f32(clip.margin))
    center = (f32(w / f32(2.0)), f32(h / f32(2.0)))
    off = (f32(f32(frame["center"][0]) * w), f32(f32(frame["center"][1]) * h))
    und = lambda k, pts: [(f32(f32(x) - off[0]), f32(f32(y) - off[1])) for x, y in mapper(k, pts)]
    with np.errstate(all="ignore"):
        polygon = und(0, rect)
        m = (f32(1000000.0), f32(f32(1000000.0) * inv_aspect))
        for rnd in range(1, 5):
            idx, m = Z.nearest_edge(polygon, center, m, inv_aspect)
            if idx is None or (variant == "break-a-round-early" and rnd == 1):
                break
            before = (119 if variant == "neighbour-119" else 15) if idx == 0 else idx - 1
            after = min(idx + 1, 119) if variant == "no-wrap" else (idx + 1) % 120
            polygon = und(rnd, Z.interpolate_points([rect[before], rect[idx], rect[after]], 30))
            _, m = Z.nearest_edge(polygon, center, m, inv_aspect)
        return float(f32(f32(m[0] * f32(2.0)) / out0))


FOLD_VARIANTS = {
    "count-strict": ["ties-all-equal", "ties-ties-across-kth", "largest-pair-all-equal", "largest-pair-two-values", "frame-46340"],
    "no-remainder": ["ties-all-equal", "ties-ties-across-kth", "ties-ties-end-at-k", "largest-pair-two-values", "count-10+0-opencv_standard"],
    "k-rounded": ["count-11+0-opencv_standard", "count-64+3-opencv_standard", "count-65+8-opencv_standard", "compact-64-of-128", "largest-pair-all-equal"],
    "bounds-inclusive": ["on-and-inside-the-edges", "count-9+3-opencv_standard", "count-10+8-poly5", "compact-65-of-129"],
    "signed-compare": ["frame-46340"],
}


def test_the_restated_fold_equals_the_statement_on_every_case():
    for case in COSTS.values():
        want = T.precondition_sync(case)
        for c in range(len(case.candidates)):
            assert model_cost(case, c) == want[c], (case.name, c)


@pytest.mark.parametrize("variant", list(FOLD_VARIANTS))
def test_a_wrong_fold_changes_the_cases_it_names(variant):
    for name in FOLD_VARIANTS[variant]:
        case = COSTS[name]
        assert model_cost(case, 0, variant) != T.precondition_sync(case)[0], (variant, name)


@pytest.mark.parametrize("variant", ["first-minimum", "no-cross-lane-tie-break"])
def test_a_wrong_reduce_changes_every_search(variant):
    for case in SEARCHES.values():
        st = T.precondition_search(case)
        assert model_pick(st["coarse_costs"]) == st["coarse_pick"] == SS.find_min(st["coarse_costs"]), case.name
        assert model_pick(st["coarse_costs"], variant) != st["coarse_pick"], (variant, case.name)
        assert model_pick(st["fine_costs"]) == st["fine_pick"] and model_pick(st["fine_costs"], "first-minimum") != st["fine_pick"]


ZOOM_VARIANTS = {"neighbour-119": ["tilt-1.5+2.5-roll+0.1", "tilt-1+2-roll-0.05"], "no-wrap": ["tilt-1+5-roll-0.5"],
                 "break-a-round-early": ["roll+1", "roll-5", "tilt+3+2", "shear+0.01"]}


def test_the_restated_rounds_equal_the_statement_on_every_frame():
    for group in GROUPS.values():
        st = T.precondition_zoom(group)
        got = np.array([model_find_fov(group, f) for f in group.frames])
        assert T.same_bits(got, st["fov"]), group.name


@pytest.mark.parametrize("variant", list(ZOOM_VARIANTS))
def test_a_wrong_round_loop_changes_the_frames_it_names(variant):
    group = GROUPS["16:9"]
    st = T.precondition_zoom(group)
    names = [f["name"] for f in group.frames]
    for name in ZOOM_VARIANTS[variant]:
        k = names.index(name)
        assert model_find_fov(group, group.frames[k], variant) != st["fov"][k], (variant, name)
