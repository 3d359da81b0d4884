"""TEST INFRASTRUCTURE: one case table of plain data for the sync fold / reduce and the zoom rounds on TABULATED points, through the PUBLIC entry points
(gfw_sync_visual_costs, gfw_sync_visual_search, gfw_zoom_fovs) on both kernel tiers.  Not a product path.

The lens that makes a table of points its own table of mapped points (every step exact in f32, or one correctly rounded operation both sides perform):
  * opencv_standard with every k zero: icdist = 1 / 1, no tangential terms, x = px; a NaN stays a NaN.  poly5 with k = 0: px * (rd / rd) — and None exactly
    at the principal point, the one way to a rejected ray ((-1e6, -1e6), cpu_undistort.rs:855) from finite input (a NaN input is rejected as well);
  * f = (128, 128), c = (w / 2, h / 2) = new_k's: (x - c) / 128 and 128 * ptx + c are exact for the coordinates used here (multiples of 1/64 below 512, 2^-15 next to
    0 / w / h, whole pixels of the 46340 x 46340 frame), pr2 = 1; no digital lens, stretches and refraction 1;
  * quaternions with entries 0 and +-1: the identity and the three half-turns.  Their self-dot is 1 (slerp between two equal keys returns the first), with
    smoothed == org the prefix smoothed * org^-1 is the exact identity, R and new_k * R are exact.  The half-turn about z maps x -> 2 c - x.
Every case names the branch it is there for and carries its precondition, checked on the statements alone (precondition_*) BEFORE a kernel output is looked at."""
import numpy as np

from gyroflow_amd import abi
import _hoststmt as H
import _synccase as SC
import _syncstmt as SS
import _zoomstmt as Z

f32 = np.float32
W, HT = 320, 180
BIG = 46340                                    # 46340 x 46341 is the largest frame gfw_sync_visual_* accept
IDENT, HALF_X, HALF_Y, HALF_Z = (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)
NONE = -1000000.0


def same_bits(a, b):
    """uint32 / uint64 views agree; NaN compares as NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def track_of(quats):
    """keys 1 ms apart, in whole microseconds, from 0 on"""
    q = np.array(quats, dtype=np.float64).reshape(-1, 4)
    return np.arange(len(q), dtype=np.int64) * 1000, q


class TableClip(Z.Clip):
    """a statement clip with the identity lens, and ONE track given as plain data for org and smoothed alike; counts the lookups that fall between unequal keys"""

    def __init__(self, name, model="opencv_standard", size=(W, HT), out=None, margin=0.0, track=None):
        lens = {"model": model, "f": (128.0, 128.0), "c": (size[0] / 2.0, size[1] / 2.0), "k": [0.0] * 12, "r_limit": 0.0}
        Z.Clip.__init__(self, name, lens=lens, size=size, out=out or size, margin=margin, frames=1)
        self.timestamps = [0.0]
        self._track = track if track is not None else track_of([IDENT] * 3)
        self.unequal_lookups = 0

    @property
    def tracks(self):
        return self._track, self._track

    def on_lookup(self, track, timestamp_ms, offsets, duration_ms):
        ts, q = track
        if len(ts) < 2 or not duration_ms > 0.0:
            return
        t = timestamp_ms - H.offset_at(offsets, timestamp_ms)
        lookup = max(min(H._as_i64(H._round(t * 1000.0)), int(ts[-1])), int(ts[0]))
        i = int(np.searchsorted(ts, lookup, side="right")) - 1
        if ts[i] != lookup and i + 1 < len(ts) and not np.array_equal(q[i], q[i + 1]):
            self.unequal_lookups += 1

    def quat_at(self, track, timestamp_ms):
        self.on_lookup(track, timestamp_ms, self.sync_offsets, self.duration_ms)
        return Z.Clip.quat_at(self, track, timestamp_ms)


# ================================================================================================ visual-features costs
KINDS = ("edge", "outside", "nan", "given-none", "lens-none")


class SyncCase:
    """pairs [(ts_us, next_ts_us, p [n][2], q [n][2])] handed to the entry point, candidates [(offs, readout)], and per candidate the table the mapped output must
    equal to the bit (`expected`: [n_cand][total][2][2]).  k: per pair the expected (n_valid as f64 * 0.9) as usize; rejects: rows of the call per kind."""

    def __init__(self, name, branch, clip, pairs, k, rejects=None, candidates=((0.0, 0.0),), expected=None, more=None):
        self.name, self.branch, self.clip, self.k, self.more = name, branch, clip, list(k), more or {}
        self.range = SS.Range(clip, pairs)
        self.candidates = [(float(o), float(r)) for o, r in candidates]
        self.rejects = dict({kind: 0 for kind in KINDS}, **(rejects or {}))
        if expected is None:
            t = np.concatenate([np.stack([p, q], 1) for _, _, p, q in self.range.pairs]) if self.range.total else np.zeros((0, 2, 2), np.float32)
            c = np.array(clip.lens["c"], dtype=np.float32)
            if clip.lens["model"] == "poly5":
                t[(t == c).all(axis=2)] = NONE                                   # the lens's None
            t[np.isnan(t).any(axis=2)] = np.nan                                  # r2 is NaN: both coordinates of that side (a NaN row compares as NaN)
            expected = [t] * len(self.candidates)
        self.expected = np.array(expected, dtype=np.float32).reshape(len(self.candidates), self.range.total, 2, 2)

    @property
    def pairs(self):
        return self.range.pairs

    def search(self):
        return SC.sync_search(self.clip)

    def table_of_pairs(self, c=0):
        """the expected mapped points of candidate c, pair by pair"""
        out, at = [], 0
        for _, _, p, _ in self.pairs:
            out.append(self.expected[c][at:at + len(p)])
            at += len(p)
        return out


def classify(case, c=0):
    """-> (n_valid per pair, rows per reject kind) of the expected table of candidate c, by the bounds test of visual_features.rs:68-69 read off the plain numbers"""
    w, h = case.clip.size
    rejects = {kind: 0 for kind in KINDS}
    n_valid, at = [], 0
    for _, _, p, q in case.pairs:
        given = np.stack([p, q], 1)
        valid = 0
        for row, src in zip(case.expected[c][at:at + len(p)], given):
            if np.isnan(row).any():
                rejects["nan"] += 1
            elif (row == NONE).all(axis=1).any():
                rejects["given-none" if (src == NONE).all(axis=1).any() else "lens-none"] += 1
            elif (row[:, 0] < 0).any() or (row[:, 0] > w).any() or (row[:, 1] < 0).any() or (row[:, 1] > h).any():
                rejects["outside"] += 1
            elif (row[:, 0] == 0).any() or (row[:, 0] == w).any() or (row[:, 1] == 0).any() or (row[:, 1] == h).any():
                rejects["edge"] += 1
            else:
                valid += 1
        n_valid.append(valid)
        at += len(p)
    return n_valid, rejects


def distances(case, c=0):
    """per pair the `dist as u64` of its valid rows, from the expected table (f32 arithmetic as visual_features.rs:70-71 writes it)"""
    w, h = case.clip.size
    out = []
    for m in case.table_of_pairs(c):
        with np.errstate(all="ignore"):
            ok = ((m[:, :, 0] > 0) & (m[:, :, 0] < f32(w)) & (m[:, :, 1] > 0) & (m[:, :, 1] < f32(h))).all(axis=1)
            a, b = m[ok, 0], m[ok, 1]
            dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
            out.append(((dx * dx) + (dy * dy)).astype(np.uint64))
    return out


_SYNC_DONE = {}


def precondition_sync(case):
    """The statement alone: its mapped points of every candidate ARE the expected table (uint32 views, NaN as NaN), no lookup fell between unequal keys, k and the
    rejected rows per kind are the case's.  -> the statement's costs [n_cand] (the fold of the table)"""
    if case.name not in _SYNC_DONE:
        case.clip.unequal_lookups = 0
        for c, (offs, readout) in enumerate(case.candidates):
            got = SS.mapped_points(case.range, offs, readout)
            assert same_bits(got, case.expected[c]), (case.name, c, "the statement does not map the table onto itself")
        assert case.clip.unequal_lookups == 0, (case.name, case.clip.unequal_lookups)
        n_valid, rejects = classify(case)
        assert [int(float(n) * 0.9) for n in n_valid] == case.k, (case.name, n_valid, case.k)
        assert rejects == case.rejects, (case.name, rejects, case.rejects)
        total = sum(len(p) for _, _, p, _ in case.pairs)
        for key, (lo, hi) in case.more.get("rejected_share", {}).items():
            n = len(case.pairs[key][2])
            assert lo <= 1.0 - n_valid[key] / float(n) <= hi, (case.name, key, n_valid[key], n)
        if "n_valid" in case.more:
            assert n_valid == case.more["n_valid"], (case.name, n_valid)
        if "at_or_above_2_31" in case.more:
            d = distances(case)[0]
            hi, lo = int((d >= 2 ** 31).sum()), int((d < 2 ** 31).sum())
            assert hi >= case.more["at_or_above_2_31"] and lo >= case.more["below_2_31"], (case.name, hi, lo)
            assert int(np.sort(d)[case.k[0] - 1]) >= 2 ** 31, case.name
        if "kth_inside_run_of" in case.more:                                         # the cut falls inside the run of this value, in this pair
            key, value = case.more["kth_inside_run_of"]
            d = np.sort(distances(case)[key])
            k = case.k[key]
            assert d[k - 1] == value and d[k] == value and d[0] < value, (case.name, d[k - 1], d[k])
        assert total == case.range.total
        _SYNC_DONE[case.name] = [SS.fold_mapped(case.range, case.expected[c]) for c in range(len(case.candidates))]
    return _SYNC_DONE[case.name]


def _valid_rows(dists, g, size=(W, HT)):
    """point pairs a whole dx (and dy) apart, so that the distance is the integer dx^2 + dy^2 exactly: d a perfect square gives d itself, any other d the nearest
    sum of two squares below it; both points share one fraction of a pixel in 1/64ths (x - c stays exact, the difference whole)"""
    rows = []
    for d in dists:
        dx = int(np.sqrt(float(d)))
        dy = int(np.sqrt(float(int(d) - dx * dx)))
        x, y = float(g.integers(4, size[0] - 4 - dx)) + float(g.integers(0, 64)) / 64.0, float(g.integers(4, size[1] - 4 - dy)) + float(g.integers(0, 64)) / 64.0
        rows.append([[x, y], [x + dx, y + dy]])
    return rows


def _reject_rows(kind, size=(W, HT)):
    w, h = float(size[0]), float(size[1])
    return {"edge": [[[0.0, 60.0], [50.0, 50.0]], [[50.0, 50.0], [w, 60.0]], [[50.0, h], [50.0, 50.0]], [[50.0, 0.0], [51.0, 50.0]]],
            "outside": [[[50.0, 50.0], [w + 1.0, 50.0]], [[-3.0, 20.0], [50.0, 50.0]], [[50.0, h + 0.5], [50.0, 50.0]]],
            "nan": [[[np.nan, 50.0], [50.0, 50.0]], [[50.0, 50.0], [50.0, np.nan]]],
            "given-none": [[[NONE, NONE], [50.0, 50.0]], [[50.0, 50.0], [NONE, NONE]]],
            "lens-none": [[[w / 2.0, h / 2.0], [50.0, 50.0]], [[50.0, 50.0], [w / 2.0, h / 2.0]]]}[kind]


def _with_rejects(valid, n_rejected, g, kinds, size=(W, HT), interleave=False):
    """-> (rows [n][2][2] f32 shuffled — or the rejected rows dealt evenly between the valid ones —, rows per kind)"""
    counts = {kind: 0 for kind in kinds}
    bad = []
    for j in range(n_rejected):
        kind = kinds[j % len(kinds)]
        forms = _reject_rows(kind, size)
        bad.append(forms[(j // len(kinds)) % len(forms)])
        counts[kind] += 1
    rows = list(valid) + bad
    m = np.array(rows, dtype=np.float32).reshape(-1, 2, 2)
    if interleave and len(bad) and len(valid):
        order = np.argsort(np.concatenate([np.arange(len(valid)) / float(len(valid)), (np.arange(len(bad)) + 0.5) / float(len(bad))]), kind="stable")
        return m[order], counts
    return (m[g.permutation(len(m))] if len(m) else m), counts


def _pair(m, k=0):
    """a table [n][2][2] as the k-th pair of a call: frames 33 ms apart (the constant track makes the time immaterial)"""
    m = np.asarray(m, dtype=np.float32).reshape(-1, 2, 2)
    return (1000000 + 400000 * k, 1033000 + 400000 * k, m[:, 0].copy(), m[:, 1].copy())


CVSTD_KINDS = ("edge", "outside", "nan", "given-none")
POLY5_KINDS = ("lens-none", "edge", "given-none", "outside")
K_OF = {0: 0, 1: 0, 9: 8, 10: 9, 11: 9, 64: 57, 65: 58, 70: 63}      # (n as f64 * 0.9) as usize


def sync_cost_cases():
    cases = []
    flat = TableClip("identity-cvstd")
    poly = TableClip("identity-poly5", model="poly5")
    # ---- fold counts (tests/test_emu_sync.py::test_fold_counts), as input points
    for nv in sorted(K_OF):
        for inv in ((0, 3, 8, 70) if nv else (3, 8, 70)):
            for clip, kinds in ((flat, CVSTD_KINDS),) + (((poly, POLY5_KINDS),) if nv in (10, 65) and inv else ()):
                g = np.random.default_rng(1000 * nv + inv)
                m, counts = _with_rejects(_valid_rows(g.integers(0, 30, nv) ** 2, g), inv, g, kinds)
                cases.append(SyncCase("count-%d+%d-%s" % (nv, inv, clip.lens["model"]), "k = %d of %d valid among %d rejected rows" % (K_OF[nv], nv, inv), clip,
                                      [_pair(m)], [K_OF[nv]], counts))
    # ---- ties and integer edges (test_fold_ties_and_integer_edges)
    g = np.random.default_rng(7)
    ties = {"all-equal": ([25] * 40, 36), "all-zero": ([0] * 33, 29), "ties-across-kth": ([1] * 5 + [9] * 30 + [400] * 5, 36), "ties-end-at-k": ([4] * 18 + [16] * 2, 18),
            "one-large": ([0] * 9 + [90000], 9), "random-ties": (list(g.integers(0, 12, 200) ** 2), 180), "wide": (list(g.integers(0, 60000, 150)), 135)}
    for what, (d, k) in ties.items():
        m, counts = _with_rejects(_valid_rows(d, g), 4, g, CVSTD_KINDS)
        cases.append(SyncCase("ties-" + what, "the bisection's count at T, the (k - cnt_below) * T term: " + what, flat, [_pair(m)], [k], counts))
    below = 2.0 - 2.0 ** -12                                                      # dx^2 = 4 - 2^-10 + 2^-24 rounds to 3.9990234: `as u64` 3; dx = 2 gives 4
    m = np.array([[[10.0, 10.0], [10.0 + d, 10.0]] for d in [below] * 10 + [2.0] * 10], dtype=np.float32)
    cases.append(SyncCase("just-below-an-integer", "`dist as u64` truncates: 3.999 -> 3 beside 4.0 -> 4", flat, [_pair(m)], [18], more={"n_valid": [20]}))
    e = 2.0 ** -15                                                                # (nextafter(0, 1) - c is not representable; 2^-15 and w - 2^-15 are)
    inside = [[[e, 5.0], [W - e, HT - e]]] * 10
    edge = [[[0.0, 5.0], [9.0, 5.0]], [[5.0, 0.0], [9.0, 5.0]], [[float(W), 5.0], [9.0, 5.0]], [[5.0, float(HT)], [9.0, 5.0]], [[9.0, 5.0], [5.0, float(HT)]]]
    cases.append(SyncCase("on-and-inside-the-edges", "strict bounds: exactly 0, w, h rejected, 2^-15 inside kept", flat, [_pair(np.array(inside + edge, dtype=np.float32))], [9],
                          {"edge": 5}, more={"n_valid": [10]}))
    # ---- compaction across batches of 64 lanes: rejected rows dealt between the valid ones
    shapes = [(63, 30), (64, 32), (65, 33), (128, 64), (129, 65), (200, 128), (200, 64)]
    tables = []
    for n, nv in shapes:
        g = np.random.default_rng(n * 1000 + nv)
        m, counts = _with_rejects(_valid_rows(g.integers(0, 40, nv) ** 2 if n % 2 else g.integers(0, 60000, nv), g), n - nv, g, CVSTD_KINDS, interleave=True)
        tables.append((m, counts))
        cases.append(SyncCase("compact-%d-of-%d" % (nv, n), "rank offset n_valid + mbcnt over %d batches, %d valid" % ((n + 63) // 64, nv), flat, [_pair(m)], [int(float(nv) * 0.9)],
                              counts, more={"n_valid": [nv], "rejected_share": {0: (0.3, 0.7)}}))
    total = {kind: sum(c.get(kind, 0) for _, c in tables) for kind in CVSTD_KINDS}
    cases.append(SyncCase("compact-all-pairs", "the seven compaction pairs in one call", flat, [_pair(m, k) for k, (m, _) in enumerate(tables)],
                          [int(float(nv) * 0.9) for _, nv in shapes], total, more={"n_valid": [nv for _, nv in shapes], "rejected_share": {k: (0.3, 0.7) for k in range(7)}}))
    # ---- the largest pair decides the dynamic LDS size: behind a pair of 3, in front of pairs of 0 and 130 points
    for what, d, more in (("all-equal", [49] * 4096, {}), ("two-values", [4] * 3000 + [25] * 1096, {"kth_inside_run_of": (1, 25)})):
        g = np.random.default_rng(4096)
        big = np.array(_valid_rows(d, g), dtype=np.float32)[g.permutation(4096)]
        small, tail = np.array(_valid_rows([1, 4, 9], g), dtype=np.float32), np.array(_valid_rows(g.integers(0, 20, 130) ** 2, g), dtype=np.float32)
        cases.append(SyncCase("largest-pair-" + what, "4096 valid rows fill the dynamic LDS block, sized from the call's largest pair: " + what, flat,
                              [_pair(small, 0), _pair(big, 1), _pair(np.zeros((0, 2, 2)), 2), _pair(tail, 3)], [2, 3686, 0, 117], more=dict(more, n_valid=[3, 4096, 0, 130])))
    # ---- distances of 2^31 and more: an unsigned compare, the bisection from hi = 0xffffffff
    large = TableClip("identity-46340", size=(BIG, BIG))
    g = np.random.default_rng(31)
    rows = []
    for i in range(12):                                                           # 40000^2 + 30000^2 = 2.5e9 and thereabouts, three runs of four: ties across the k-th
        x, y = float(g.integers(10, 3000)), float(g.integers(10, 3000))
        rows.append([[x, y], [x + 40000.0 + 16.0 * (i // 4), y + 30000.0]])
    for i in range(12):                                                           # 1.25e9 and below
        x, y = float(g.integers(10, 3000)), float(g.integers(10, 3000))
        rows.append([[x, y], [x + 25000.0 + 100.0 * (i // 2), y + 25000.0 - 2000.0 * i]])
    m, counts = _with_rejects(rows, 4, g, ("edge", "outside"), size=(BIG, BIG))
    cases.append(SyncCase("frame-46340", "u32 distances at and above 2^31; bound (w^2 + h^2) * 1.001 + 1 >= 2^32 - 256: hi = 0xffffffff", large, [_pair(m)], [21], counts,
                          more={"n_valid": [24], "at_or_above_2_31": 10, "below_2_31": 10}))
    # ---- rolling shutter: rows of one pair on different plateaus, carried across a plateau boundary by row_readout_time * y
    cases.append(_rolling_case())
    return cases


def _plateau_flip(q, p, size=(W, HT)):
    """what the plateau's quaternion does to a mapped point"""
    x, y = float(p[0]), float(p[1])
    fx = q in (HALF_Z, HALF_X)
    fy = q in (HALF_Z, HALF_Y)
    return [size[0] - x if fx else x, size[1] - y if fy else y]


def _rolling_case():
    """keys 0 .. 1399 ms: identity, a half-turn about z over [1000, 1200), the half-turn about x from 1300 on.  Pair at 1000 / 1250 ms; a row's time is
    ts - offs - frt / 2 + frt / 180 * y: whole or half milliseconds for whole rows, so every lookup lies on a key or between two equal keys as long as no time falls
    strictly between 999 and 1000, 1199 and 1200 or 1299 and 1300 (asserted by the lookup count)"""
    kinds = [IDENT] * 1000 + [HALF_Z] * 200 + [IDENT] * 100 + [HALF_X] * 100
    clip = TableClip("plateaus-rolling", track=track_of(kinds))
    cands = [(0.0, 90.0), (0.0, -90.0), (20.0, 180.0), (-100.0, 90.0), (0.0, 0.0)]
    g = np.random.default_rng(90)
    ys = np.array([y for y in range(6, 176, 3) if y not in (89, 109)], dtype=np.float64)
    p = np.stack([g.integers(8, 150, len(ys)).astype(np.float64) + 0.25, ys], 1)
    q = p + np.stack([g.integers(0, 4, len(ys)), np.zeros(len(ys))], 1)          # the same row on both sides, 0 .. 3 px apart
    expected, crossing = [], 0
    for offs, frt in cands:
        rows = []
        for a, b in zip(p, q):
            sides = []
            for ts, pt in ((1000.0, a), (1250.0, b)):
                t = ts - offs - frt / 2.0 + frt / 180.0 * pt[1] if frt else ts - offs
                assert t == np.floor(t * 2.0) / 2.0
                sides.append(kinds[int(np.floor(t))])                            # between two keys: both are the plateau's (the lookup count holds this to account)
            rows.append([_plateau_flip(sides[0], a), _plateau_flip(sides[1], b)])
            crossing += sides[0] != sides[1]
        expected.append(rows)
    case = SyncCase("rolling-plateaus", "rolling shutter: the rows of one pair look up different plateaus", clip, [(1000000, 1250000, p, q)], [int(float(len(ys)) * 0.9)],
                    candidates=cands, expected=expected, more={"n_valid": [len(ys)]})
    assert 50 < crossing < len(cands) * len(ys) - 50                              # some rows of every kind: both sides on one plateau, and on two
    return case


# ================================================================================================ visual-features search
class SearchCase:
    def __init__(self, name, branch, clip, pairs, mode, minima, initial_offset=0.0, search_size=0.0, readout=0.0, fps=30.0):
        self.name, self.branch, self.clip, self.mode, self.minima = name, branch, clip, mode, minima
        self.range = SS.Range(clip, pairs)
        self.args = dict(initial_offset=initial_offset, search_size=search_size, readout=readout, fps=fps)

    @property
    def pairs(self):
        return self.range.pairs

    def search(self):
        return SC.sync_search(self.clip)


def lane_of(i):
    return i % 256


def _search_pairs(seed, sizes, gap_ms):
    """points in the upper left quarter, 0 .. 3 px apart: a half-turn about z on ONE side sends that side to the lower right quarter — a large, designed distance"""
    g = np.random.default_rng(seed)
    pairs = []
    for n in sizes:
        p = np.stack([g.integers(16, 120, n), g.integers(12, 70, n)], 1).astype(np.float64) + 0.5
        q = p + np.stack([g.integers(0, 4, n), g.integers(0, 3, n)], 1)
        pairs.append((1000000, 1000000 + gap_ms * 1000, p, q))
    return pairs


TIE_RUNS = [(16, 18), (298, 300), (455, 457), (597, 599)]      # runs of equal minima of the 600-candidate search; the last ends at the last candidate (see search_cases)


def search_cases():
    """Whole-millisecond coarse candidates i put side A of every pair on key 1300 - i and side B on key 2000 - i.  The track is the identity but for the half-turn
    about z on B's keys of every candidate outside TIE_RUNS, so exactly the candidates of TIE_RUNS have both sides on equal plateaus and the table's own cost.
    The fine stage looks up between keys: with no lookup between unequal keys allowed, the three keys around each side of the coarse pick are equal, so the
    candidates next to the pick cost what it costs — the last minimum of a coarse stage whose fine stage is exact is therefore its last candidate, and the runs are
    three wide.  Lanes of the 256-lane reduce: 16-18 and 42-44 (strides 0, 1), 199-201 (stride 1), 85-87 (stride 2): the pick, 599, sits in lane 87, not the highest."""
    kinds = [IDENT] * 2101
    minima = [i for a, b in TIE_RUNS for i in range(a, b + 1)]
    for i in range(600):
        if i not in minima:
            kinds[2000 - i] = HALF_Z
    ties = TableClip("plateaus-ties", track=track_of(kinds))
    const = TableClip("plateaus-constant", track=track_of([HALF_Y] * 40))
    return [SearchCase("ties-600", "equal minima in lanes 16-18, 42-44, 199-201 and 85-87 of the reduce: the last index wins, not the highest lane", ties,
                       _search_pairs(1, [10, 70], 700), 0, minima, search_size=600.0),
            SearchCase("all-equal-520", "every cost equal over more than two strides: the last candidate", const, _search_pairs(2, [9, 65], 33), 0, list(range(520)),
                       initial_offset=3.0, search_size=520.0),
            SearchCase("all-equal-readout", "mode 1, every cost equal: 666 rolling-shutter candidates on a constant track", const, _search_pairs(3, [7, 12], 33), 1,
                       list(range(666)), fps=3.0)]


_SEARCH_DONE = {}


def precondition_search(case):
    """-> the statement's search (dict of _syncstmt.search); asserts the equal minima, the pick and that no lookup fell between unequal keys"""
    if case.name not in _SEARCH_DONE:
        case.clip.unequal_lookups = 0
        st = SS.search(case.range, case.mode, **case.args)
        assert case.clip.unequal_lookups == 0, (case.name, case.clip.unequal_lookups)
        cc = st["coarse_costs"]
        assert [i for i, c in enumerate(cc) if c == min(cc)] == case.minima and len(case.minima) >= 3, (case.name, [i for i, c in enumerate(cc) if c == min(cc)][:20])
        assert st["coarse_pick"] == case.minima[-1] == len(cc) - 1 and st["fine_pick"] == 199 and len(set(st["fine_costs"])) == 1
        lanes = sorted({lane_of(i) for i in case.minima})
        assert len(lanes) >= 3 and len({i // 256 for i in case.minima}) >= 3 and lane_of(case.minima[-1]) < lanes[-1], (case.name, lanes)
        if case.name == "ties-600":
            assert len(cc) >= 600 and min(cc) > 0.0 and sorted(set(cc))[1] > 100.0 * min(cc)
        _SEARCH_DONE[case.name] = st
    return _SEARCH_DONE[case.name]


def check_search(case, res, coarse_costs, fine_costs, fine=None):
    """a tier's search against the statement's, to the bit"""
    st = precondition_search(case)
    col = 0 if case.mode == 0 else 1
    f64 = lambda v: np.array(v, dtype=np.float64)
    assert res.found == 1 and res.n_coarse == len(st["coarse"])
    assert same_bits(f64(coarse_costs), f64(st["coarse_costs"])), case.name
    assert same_bits(f64(fine_costs), f64(st["fine_costs"])), case.name
    assert same_bits(f64([res.coarse_value, res.coarse_cost, res.value, res.cost]),
                     f64([st["coarse"][st["coarse_pick"]][col], st["coarse_costs"][st["coarse_pick"]], st["value"], st["cost"]])), (case.name, res.coarse_value, res.value)
    if fine is not None:
        assert same_bits(f64(fine).reshape(-1, 2), f64(st["fine"])), case.name


# ================================================================================================ zoom search
class ZoomGroup:
    """frames of one gfw_zoom_fovs call: they share the lens, the sizes and the margin.  frames: [dict(name, branch, rot [9] f32, center, exit, first, side)] —
    exit / first: the expected way out of the loop and index of the first fold, or None: found with the statement and only counted"""

    def __init__(self, name, model, out, margin, frames, size=(W, HT)):
        self.name, self.frames = name, frames
        self.clip = TableClip("zoom-" + name, model=model, size=size, out=out, margin=margin)

    def inputs(self, order=None):
        """-> (KernelParams, abi.ZoomSearch, ctypes frames, rotations [n][9] f32) in the given order of frames"""
        clip = self.clip
        order = list(range(len(self.frames))) if order is None else list(order)
        kp = clip.kernel_params()
        kp.lens_correction_amount, kp.fov = 1.0, 0.0
        search = abi.ZoomSearch(width=clip.size[0], height=clip.size[1], org_output_width=clip.out[0], org_output_height=clip.out[1], fov_algorithm_margin=clip.margin,
                                horizontal_readout=0)
        frames = (abi.ZoomFrame * len(order))()
        nk = np.asarray(clip.new_k(), dtype=np.float64).reshape(9)
        for j, k in enumerate(order):
            f = frames[j]
            f.timestamp_ms, f.per_frame_time_offset_ms, f.frame_readout_time_ms = 1000.0 + j, 0.0, 0.0
            for i in range(9):
                f.new_k[i] = nk[i]
            f.fov, f.video_rotation_deg, f.lens_correction_amount, f.suppress_rotation = 1.0, 0.0, 1.0, 0
            f.zoom_center[0], f.zoom_center[1] = self.frames[k]["center"]
        return kp, search, frames, np.array([self.frames[k]["rot"] for k in order], dtype=np.float32).reshape(-1, 9)


def _k_times(r, size=(W, HT)):
    """new_k * R, rounded once to f32, as plain numbers"""
    nk = np.array([[128.0, 0.0, size[0] / 2.0], [0.0, 128.0, size[1] / 2.0], [0.0, 0.0, 1.0]])
    return [float(v) for v in (nk @ np.asarray(r, dtype=np.float64)).astype(np.float32).reshape(9)]


def _roll(deg):
    a = np.radians(deg)
    return [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]


def _tilt(deg_x, deg_y):
    a, b = np.radians(deg_x), np.radians(deg_y)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    return rx @ ry


def _frame(name, branch, rot, center=(0.0, 0.0), exit=None, first=None):
    return dict(name=name, branch=branch, rot=rot, center=center, exit=exit, first=first)


def zoom_frames(size=(W, HT)):
    """the frames every group runs (their exits differ with the aspect and the margin: only the main group states them)"""
    fr = [_frame("identity", "the corner is accepted and every later point ties: idx 0, its neighbours 15, 0, 1", _k_times(np.eye(3), size), exit="second-none", first=0)]
    for deg in (0.5, 1.0, 2.0, 3.5, 5.0):
        for s in (1.0, -1.0):
            fr.append(_frame("roll%+g" % (s * deg), "a small roll: the refinement finds a nearer point", _k_times(_roll(s * deg), size), exit="second-some"))
    for ax, ay in ((4.0, 0.0), (-4.0, 0.0), (0.0, 4.0), (0.0, -4.0), (3.0, 2.0), (-2.0, 3.0), (2.0, -3.0), (-3.0, -2.0), (7.0, 0.0), (0.0, -7.0)):
        fr.append(_frame("tilt%+g%+g" % (ax, ay), "a perspective tilt pulls one side in", _k_times(_tilt(ax, ay), size)))
    for ax, ay, deg in ((3.0, 0.0, 1.0), (-3.0, 0.0, -1.0), (0.0, 3.0, 2.0), (0.0, -3.0, -2.0), (5.0, 1.0, 0.5), (-1.0, 5.0, -0.5), (1.0, -5.0, 3.0), (-5.0, -1.0, -3.0),
                        (-1.5, 2.5, 0.1), (-1.0, 2.0, -0.05)):
        fr.append(_frame("tilt%+g%+g-roll%+g" % (ax, ay, deg), "tilt and roll", _k_times(_tilt(ax, ay) @ np.array(_roll(deg)), size),
                         first={(-1.0, 5.0, -0.5): 119, (-1.5, 2.5, 0.1): 0, (-1.0, 2.0, -0.05): 0}.get((ax, ay, deg))))
    # (the frames that end their first fold at idx 119 — the (idx + 1) % 120 wrap — and at idx 0 with a result that depends on the `15` neighbour were found with the
    # statement; their first index is asserted on its trace)
    for sh in (0.002, -0.002, 0.01, -0.01, 0.05, -0.05):
        fr.append(_frame("shear%+g" % sh, "a sheared outline", _k_times([[1.0, sh, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], size)))
        fr.append(_frame("shear-y%+g" % sh, "a sheared outline", _k_times([[1.0, 0.0, 0.0], [sh, 1.0, 0.0], [0.0, 0.0, 1.0]], size)))
    for cz in ((0.004, 0.0), (-0.004, 0.0), (0.0, 0.004), (0.0, -0.004), (0.03, -0.02), (-0.05, 0.04), (0.001, 0.001), (-0.001, -0.001)):
        fr.append(_frame("centre%+g%+g" % cz, "a zoom-centre offset", _k_times(np.eye(3), size), center=cz))
        fr.append(_frame("centre%+g%+g-roll1" % cz, "a zoom-centre offset under a roll", _k_times(_roll(1.0), size), center=cz))
    for sc in (0.9, 0.97, 1.03, 1.2):
        fr.append(_frame("scale%g" % sc, "a scaled outline: every edge point ties or the corner wins", _k_times(np.diag([sc, sc, 1.0]), size)))
    for j, far in enumerate((3.0e6, -3.0e6, 1.0e7, 5.0e8, 1.0e30, -2.0e9)):
        rot = _k_times(np.eye(3), size)
        rot[2], rot[5] = far, (far if j % 2 else -far)
        fr.append(_frame("far%g" % far, "every point beyond 1e6: nothing accepted, fov_minimal = 2e6 / out_w exactly", rot, exit="none"))
    for j in range(9):
        if j in (6, 7):
            continue
        rot = _k_times(_roll(1.0), size)
        rot[j] = float("nan")
        fr.append(_frame("nan-entry-%d" % j, "a NaN entry: every compare false, the polygon holds NaN", rot, exit="none"))
    return fr


def zoom_groups():
    groups = [ZoomGroup("16:9", "opencv_standard", (W, HT), 0.0, zoom_frames()),
              ZoomGroup("4:3", "opencv_standard", (240, 180), 0.0, zoom_frames()[::3]),
              ZoomGroup("9:16", "opencv_standard", (180, 320), 0.0, zoom_frames()[1::3]),
              ZoomGroup("2560:1080", "opencv_standard", (2560, 1080), 0.0, zoom_frames()[2::3]),
              ZoomGroup("margin2", "opencv_standard", (W, HT), 2.0, zoom_frames()[::2]),
              ZoomGroup("poly5-4:3-margin2", "poly5", (240, 180), 2.0, zoom_frames()[1::4]),
              ZoomGroup("poly5", "poly5", (W, HT), 0.0, [f for f in zoom_frames() if f["name"].startswith(("centre", "identity", "roll", "far"))])]
    return groups


def side_of(idx):
    return ("top", "right", "bottom", "left")[idx // 30]


_ZOOM_DONE = {}


def precondition_zoom(group):
    """the statement alone -> dict(fov [n] f64, debug [n][120][2] f64, traces, exits, polygons): each frame's stated exit and first index hold; polygons: per frame
    what the statement's map returned for the outline and for the refinement (for the table route of the interpreter)"""
    if group.name not in _ZOOM_DONE:
        clip = group.clip
        fov, dbg, traces, exits, polygons = [], [], [], [], []
        for f in group.frames:
            tr, seen = [], {}
            mapper = Z.mapper_for(clip, 0, rotation=np.array(f["rot"], dtype=np.float32))

            def watched(k, pts, mapper=mapper, seen=seen):
                seen[k] = mapper(k, pts)
                return seen[k]
            v, d = Z.find_fov(watched, clip.size[0], clip.size[1], clip.out, clip.margin, f["center"], tr)
            ex = "none" if not tr else "second-none" if tr[0][2] is None else "second-some"
            assert len(tr) <= 1, (group.name, f["name"], tr)
            if f["exit"] is not None and group.name == "16:9":
                assert ex == f["exit"], (group.name, f["name"], ex, tr)
            if f["first"] is not None and group.name == "16:9":
                assert tr[0][1] == f["first"], (group.name, f["name"], tr)
            if f["name"].startswith("far"):
                assert ex == "none" and v == float(f32(f32(2000000.0) / f32(f32(clip.out[0]) * f32(f32(clip.size[0]) / f32(clip.out[0]))))), (group.name, f["name"], v)
            if f["name"].startswith("nan"):
                assert ex == "none" and np.isnan(d).any(), (group.name, f["name"])
            fov.append(v); dbg.append(d); traces.append(tr); exits.append(ex); polygons.append(seen)
        _ZOOM_DONE[group.name] = dict(fov=np.array(fov), debug=np.array(dbg), traces=traces, exits=exits, polygons=polygons)
    return _ZOOM_DONE[group.name]


def precondition_zoom_table(groups):
    """over the whole table: each exit at least five times, idx 0 and idx 119 reached, a refinement that finds a nearer point at each of the four sides"""
    exits = {"none": 0, "second-none": 0, "second-some": 0}
    firsts, sides = set(), set()
    for g in groups:
        st = precondition_zoom(g)
        for ex, tr in zip(st["exits"], st["traces"]):
            exits[ex] += 1
            if tr:
                firsts.add(tr[0][1])
                if ex == "second-some":
                    sides.add(side_of(tr[0][1]))
    assert all(v >= 5 for v in exits.values()), exits
    assert 0 in firsts and 119 in firsts, sorted(firsts)
    assert sides == {"top", "right", "bottom", "left"}, sides
    assert max(len(g.frames) for g in groups) >= 65
    return exits, firsts


def shuffled(n, seed=120):
    return [int(i) for i in np.random.default_rng(seed).permutation(n)]


# ================================================================================================ gyro-match costs: queries that are no key
def gyro_nonfinite_case():
    """-> (ranges, candidates per range) for gfw_sync_gyro_costs: `(ts - offs) * 1000.0 as usize` of NaN, +-inf, +-1e300, -0.0 and a subnormal — caller-given
    candidates on two small ranges, and on the second estimated timestamps of NaN, +inf and -1e300 as well.  (Costs only: with a NaN cost in a stage,
    `if a.1 < b.1 { a } else { b }` is not associative and the pick is unspecified on either side.)"""
    import _syncgyrostmt as G
    odd = [float("nan"), float("inf"), float("-inf"), 1e300, -1e300, -0.0, 1e-320]
    a = G.make_range(40, 600, seed=3)
    e, eh, g, gh = G.make_range(8, 301, seed=5, start_ms=180.0, gyro_from_ms=100.0, fps=50.0)
    e = e.copy()
    e[1, 0], e[4, 0], e[6, 0] = float("nan"), float("inf"), -1e300
    return [a, (e, eh, g, gh)], [np.array(odd + [3.0, 12.3, -40.0]), np.array([12.3] + odd + [0.0])]
