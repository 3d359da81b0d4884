"""The sync search's kernel SOURCE (gfw_sync.hip), interpreted on the host (tests/_emu_sync.py), against the host statement (tests/_syncstmt.py) over the planted
ranges of tests/_synccase.py ("emu" shape: 3 pairs of 1, 10 and 65 points; 4 + 200 candidates a search):

(a) a cost equals the statement's fold over the call's OWN mapped points to the bit (integer arithmetic: no tolerance);
(b) the mapped points match the statement's within twice the point figure of tests/golden/sync_rotation_sensitivity.json (on the host both sides call the same libm:
    they agree to the bit here, the bar is the device test's);
(c) the statement's cost at the candidate a stage returns is at most the statement's minimum over that stage's candidates plus twice the fixture's cost figure;
(d) gfw_point_map's two halves composed equal it to the bit over the zoom statement's clips.
The fold's edge cases run on tabulated mapped points through a test-only entry of the driver (gfw_emu_sync_table), the way gfw_emu_zoom_table drives the zoom rounds."""
import numpy as np
import pytest

import _emu_sync as E
import _pairbase as PB
import _synccase as SC
import _syncstmt as SS
import _zoomstmt as Z

SENS = SC.sensitivity()
f32 = np.float32
W, H = 320, 180


def emu_args(rng):
    c = rng.clip
    return rng.kp, c.model, c.digital, SC.sync_search(c), rng.pairs


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(SC.CLIPS))
def test_costs_and_mapped_points(name, mode):
    rng, _ = SC.planted(name, "emu", mode)
    st = SC.stored(name, "emu", mode)
    coarse = SC.stage_candidates(name, "emu", mode)
    fine = SC.stage_candidates(name, "emu", mode, coarse[st["coarse_pick"]][0 if mode == 0 else 1])
    cands = [coarse[0], coarse[st["coarse_pick"]], fine[st["fine_pick"]], fine[-1]]
    costs, mapped = E.sync_visual_costs(*emu_args(rng), cands, rng.clip.tracks, mapped=True)
    for i, (offs, readout) in enumerate(cands):
        assert costs[i] == SS.fold_mapped(rng, mapped[i]), (name, mode, i)                                           # (a)
        assert float(np.max(np.abs(mapped[i] - SS.mapped_points(rng, offs, readout)))) <= 2.0 * SENS[name]["point_max_abs_px"], (name, mode, i)       # (b)
    assert costs[1] == st["coarse_costs"][st["coarse_pick"]] and costs[2] == st["cost"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(SC.CLIPS))
def test_search(name, mode):
    rng, _ = SC.planted(name, "emu", mode)
    st = SC.stored(name, "emu", mode)
    a = SC.search_args(name, "emu", mode)
    res, coarse_costs, fine_costs = E.sync_visual_search(*emu_args(rng), mode, rng.clip.tracks, a.get("initial_offset", 0.0), a.get("search_size", 0.0),
                                                         a.get("readout", 0.0), a.get("fps", 30.0))
    col = 0 if mode == 0 else 1
    coarse = SC.stage_candidates(name, "emu", mode)
    bar = 2.0 * SENS[name]["cost_max_abs"]
    assert res.found == 1 and res.n_coarse == len(coarse)
    ci = [c[col] for c in coarse].index(res.coarse_value)
    assert ci == SS.find_min(list(coarse_costs)) and res.coarse_cost == coarse_costs[ci]
    assert st["coarse_costs"][ci] - min(st["coarse_costs"]) <= bar                                                    # (c), coarse
    fine = SC.stage_candidates(name, "emu", mode, res.coarse_value)
    fi = [c[col] for c in fine].index(res.value)
    assert fi == SS.find_min(list(fine_costs)) and res.cost == fine_costs[fi]
    ref_fine = st["fine_costs"] if ci == st["coarse_pick"] else [SS.cost(rng, o, r) for o, r in fine]
    assert ref_fine[fi] - min(ref_fine) <= bar                                                                        # (c), fine


def test_sync_offsets_kept_or_cleared():
    clip = SS.PlantedClip("with-offsets", readout=12.0, track_scale=14.0)
    clip.sync_offsets, clip.duration_ms = (np.array([900000, 2500000, 4300000], dtype=np.int64), np.array([2.0, -1.5, 3.25])), 5000.0
    pairs = SC.planted("fisheye-r12", "emu", 0)[0].pairs
    cands = [(7.0, 12.0), (7.3, 0.0)]
    kept, cleared = SS.Range(clip, pairs, use_sync_offsets=True), SS.Range(clip, pairs)
    got = {}
    for use in (1, 0):
        got[use] = E.sync_visual_costs(kept.kp, clip.model, clip.digital, SC.sync_search(clip, use), pairs, cands, clip.tracks, offsets=clip.sync_offsets,
                                       duration_ms=clip.duration_ms, mapped=True)
    for use, rng in ((1, kept), (0, cleared)):
        for i, (offs, readout) in enumerate(cands):
            assert got[use][0][i] == SS.fold_mapped(rng, got[use][1][i])
            assert float(np.max(np.abs(got[use][1][i] - SS.mapped_points(rng, offs, readout)))) <= 2.0 * SENS["fisheye-r12"]["point_max_abs_px"]
    assert not np.array_equal(got[1][1], got[0][1])


@pytest.mark.parametrize("index", range(len(Z.statement_clips())))
def test_point_map_halves_compose_to_the_whole(index):
    clip = Z.statement_clips()[index]                                             # (d)
    g = np.random.default_rng(100 + index)
    w, h = clip.size
    pts = np.concatenate([np.array(Z.points_around_rect(f32(w), f32(h), f32(0.0)), dtype=np.float32),
                          np.stack([g.uniform(-0.2 * w, 1.2 * w, 200), g.uniform(-0.2 * h, 1.2 * h, 200)], 1).astype(np.float32),
                          np.array([[1e5, -1e5], [0.0, 0.0], [w / 2.0, h / 2.0]], dtype=np.float32)])
    rot = Z.point_rotations(clip, [(float(x), float(y)) for x, y in pts], 3)
    if rot.shape[0] == 1:
        rot = np.repeat(rot, len(pts), 0)
    whole, halves = E.point_split(clip.kernel_params(3), clip.model, clip.digital, pts, rot)
    assert whole.tobytes() == halves.tobytes(), clip.name
    assert np.count_nonzero(whole[:, 0] > -1000000.0) > 100, clip.name


# ------------------------------------------------------------------------------------------------ the fold on tabulated points
def table(dists, g=None, invalid=0):
    """one pair's mapped points [n][2][2] whose valid point pairs lie dx = f32(sqrt(d)) apart (a perfect square d is then the distance exactly; any other lands
    within a unit of it: the expected cost is the statement's fold of the same points either way), plus `invalid` rejected ones, shuffled"""
    g = g or np.random.default_rng(1)
    rows = []
    for d in dists:
        x, y = f32(g.integers(40, 200)), f32(g.integers(40, 120))              # whole pixels: x + dx - x = dx for a whole dx
        dx = f32(np.sqrt(f32(d)))
        rows.append([[x, y], [f32(x + dx), y]])
    for k in range(invalid):
        rows.append([[[-1000000.0, -1000000.0], [50.0, 50.0]], [[50.0, 50.0], [0.0, 60.0]], [[float(W), 60.0], [50.0, 50.0]], [[50.0, float(H)], [50.0, 50.0]],
                     [[50.0, 0.0], [51.0, 50.0]], [[50.0, 50.0], [-1000000.0, -1000000.0]], [[np.nan, 50.0], [50.0, 50.0]], [[50.0, 50.0], [float(W) + 1.0, 50.0]]][k % 8])
    m = np.array(rows, dtype=np.float32).reshape(-1, 2, 2)
    return m[g.permutation(len(m))] if len(m) else m


def run_table(pairs_mapped, candidates=None, column=0):
    """pairs_mapped: [candidate][pair] -> [n][2][2]; every candidate has the same pair sizes"""
    sizes = [len(p) for p in pairs_mapped[0]] if len(pairs_mapped) else []
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32) if sizes else np.zeros(1, np.int32)
    flat = np.array([np.concatenate(c) if sizes and sum(sizes) else np.zeros((0, 2, 2), np.float32) for c in pairs_mapped], dtype=np.float32)
    costs, res, fine = E.sync_table(flat, first, W, H, candidates, column)
    ref = [float(sum(SS.fold(p[:, 0], p[:, 1], W, H) for p in c)) for c in pairs_mapped]
    return costs, ref, res, fine


@pytest.mark.parametrize("n_valid", [0, 1, 9, 10, 11, 64, 65])
def test_fold_counts(n_valid):
    """k = (n_valid as f64 * 0.9) as usize: 0, 0, 8, 9, 9, 57, 58 — with rejected point pairs mixed in (on the frame's edge, outside, (-1e6, -1e6), NaN)"""
    g = np.random.default_rng(n_valid)
    cands = [[table(g.integers(0, 900, n_valid), g, invalid=inv)] for inv in ((0, 3, 8, 70) if n_valid else (3, 8, 70))]
    for c in cands:
        costs, ref, _, _ = run_table([c])
        assert costs[0] == ref[0], (n_valid, len(c[0]), costs, ref)
    assert int(float(n_valid) * 0.9) == {0: 0, 1: 0, 9: 8, 10: 9, 11: 9, 64: 57, 65: 58}[n_valid]


def test_fold_ties_and_integer_edges():
    g = np.random.default_rng(7)
    cases = {
        "all equal": [25] * 40,
        "all zero": [0] * 33,
        "ties across the k-th value": [1] * 5 + [9] * 30 + [400] * 5,                # k = 36: the k-th value is 400's neighbour 9 .. the cut falls inside the 9s and 400s
        "ties end exactly at k": [4] * 18 + [16] * 2,                              # k = 18
        "one large": [0] * 9 + [90000],
        "random with ties": list(g.integers(0, 12, 200) ** 2),
        "wide": list(g.integers(0, 130000, 150)),
    }
    for what, d in cases.items():
        costs, ref, _, _ = run_table([[table(d, g, invalid=4)]])
        assert costs[0] == ref[0], (what, costs, ref)
    # a distance just below and just at an integer: dx^2 = 3.9999998 truncates to 3, 4.0 to 4
    below, at = f32(np.nextafter(f32(2.0), f32(0.0))), f32(2.0)
    assert f32(below * below) < f32(4.0) and int(f32(below * below)) == 3
    m = np.array([[[10.0, 10.0], [f32(10.0) + d, 10.0]] for d in [below] * 10 + [at] * 10], dtype=np.float32)
    costs, ref, _, _ = run_table([[m]])
    assert costs[0] == ref[0] and ref[0] == float(SS.fold(m[:, 0], m[:, 1], W, H))
    # exactly on 0, w and h: excluded; one ulp inside: kept
    inside = [[[np.nextafter(f32(0.0), f32(1.0)), 5.0], [np.nextafter(f32(W), f32(0.0)), np.nextafter(f32(H), f32(0.0))]]] * 10
    edge = [[[0.0, 5.0], [9.0, 5.0]], [[5.0, 0.0], [9.0, 5.0]], [[float(W), 5.0], [9.0, 5.0]], [[5.0, float(H)], [9.0, 5.0]], [[9.0, 5.0], [5.0, float(H)]]]
    m = np.array(inside + edge, dtype=np.float32)
    costs, ref, _, _ = run_table([[m]])
    assert costs[0] == ref[0] and ref[0] > 9.0 * 100000.0                          # nine of the ten inside pairs, (w^2 + h^2) each; no edge pair


def test_fold_random_tables_over_several_pairs():
    g = np.random.default_rng(11)
    for case in range(6):
        sizes = [int(g.integers(0, 140)) for _ in range(3)] + [0]
        cands = [[table(g.integers(0, 40, n) ** 2 if case % 2 else g.integers(0, 100000, n), g, invalid=int(g.integers(0, 9))) for n in sizes] for _ in range(1)]
        costs, ref, _, _ = run_table(cands)
        assert list(costs) == ref, (case, costs, ref)


def test_reduce_picks_the_last_of_equal_minima():
    g = np.random.default_rng(3)
    pair = lambda d: [table([d] * 10, g)]                                          # cost 9 d (perfect squares: the distance is d exactly)
    cands = [pair(d) for d in (49, 9, 25, 9, 81, 9, 16)]
    values = [(10.0 + i, 2.5) for i in range(len(cands))]
    costs, ref, res, fine = run_table(cands, values, 0)
    assert list(costs) == ref == [441.0, 81.0, 225.0, 81.0, 729.0, 81.0, 144.0]
    assert res.found == 1 and res.n_coarse == 7 and res.coarse_value == 15.0 and res.coarse_cost == 81.0              # index 5: the last of the three minima
    assert [tuple(r) for r in fine] == SS.fine_candidates(0, 15.0, 2.5)
    # the same through column 1 (the readout search): 300 candidates, more than one per lane of the reduce stage, minima in different lanes
    many = [pair(4 if i in (17, 258, 299 - 256) else (9, 16, 25)[i % 3]) for i in range(300)]
    costs, ref, res, fine = run_table(many, [(0.0, float(i - 150)) for i in range(300)], 1)
    assert list(costs) == ref and res.coarse_value == float(258 - 150) and res.coarse_cost == 36.0 and res.n_coarse == 300
    assert [tuple(r) for r in fine] == SS.fine_candidates(1, float(258 - 150))


def test_no_pairs_and_no_candidates():
    costs, res, fine = E.sync_table(np.zeros((3, 0, 2, 2), np.float32), [0], W, H, [(1.0, 0.0), (2.0, 0.0), (3.0, 0.0)], 0)      # n_pairs = 0: every cost 0, the last wins
    assert list(costs) == [0.0, 0.0, 0.0] and res.found == 1 and res.coarse_value == 3.0 and res.coarse_cost == 0.0
    costs, res, fine = E.sync_table(np.zeros((0, 0, 2, 2), np.float32), [0, 0], W, H, np.zeros((0, 2)), 0)                      # steps = 0: no candidates
    assert len(costs) == 0 and res.found == 0 and res.n_coarse == 0
    rng, _ = SC.planted("fisheye-r0", "emu", 0)
    res, coarse, fine_costs = E.sync_visual_search(*emu_args(rng), 0, rng.clip.tracks, 0.0, 0.5, 0.0)                            # `0.5 as usize` = 0: five launches, nothing found
    assert res.found == 0 and len(coarse) == 0 and np.all(fine_costs == 0.0)
    assert list(E.sync_visual_costs(rng.kp, rng.clip.model, rng.clip.digital, SC.sync_search(rng.clip), [], [(0.0, 0.0), (1.0, 3.0)], rng.clip.tracks)) == [0.0, 0.0]


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged as given and the points from the arrays' start (tests/_pairbase.py)"""
    rng, cands = PB.visual()
    costs = PB.assert_base_does_not_matter(lambda: E.sync_visual_costs(*emu_args(rng), cands, rng.clip.tracks), "sync_visual_costs")
    assert len(costs) == 3 and len(set(costs.tolist())) == 3 and costs[1] == min(costs)
