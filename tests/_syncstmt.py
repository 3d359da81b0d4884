"""Host statement of the visual-features sync search (src/core/synchronization/find_offset/visual_features.rs:10-147) — the checker of
gfw_sync_visual_costs / gfw_sync_visual_search.  Test infrastructure: written from the cited Rust, independent of the device code; not part of the
product package.

  side_rotations   frame_transform.rs:376-410 (at_timestamp_for_points) = _zoomstmt.point_rotations at `timestamp - offs` with the candidate's readout time
  map_side         cpu_undistort.rs:636-641 = the oracle's undistort_points with one rotation per point, lens_correction_amount 1.0
  fold             visual_features.rs:66-81: the bounds test, `dist as u64` of the f32 squared distance, sort, the first (len as f64 * 0.9) as usize
  cost             calculate_distance (:49-83): the f64 sum over pairs (a sum of integers: exact)
  search           :87-131, both arms; `reduce_with(find_min)`, `if a.1 < b.1 { a } else { b }` under rayon's order-preserving reduce: the LAST minimal candidate

A range is a _zoomstmt.Clip (lens, size, tracks, sync offsets) with matched pairs [(ts_us, next_ts_us, points [n][2] f32, points [n][2] f32)].
No reference-produced vector exists for this path (the Rust crate cannot be built here), so tests/test_sync_statement.py holds this statement against what
the search is for — it finds a planted offset and a planted readout time — before anything is compared with it.
"""
import numpy as np

from gyroflow_amd import abi
import _hoststmt as H
import _oracle as O
import _zoomstmt as Z

f32 = np.float32
FINE = 200


class _Side:
    """the clip as at_timestamp_for_points sees it for one side of a pair: ONE frame at `timestamp - offs`, the candidate's readout time, no per-frame
    time offset; with use_sync_offsets False the gyro's offsets are cleared (visual_features.rs:13-15)"""

    def __init__(self, clip, timestamp_ms, readout, use_sync_offsets):
        self.size, self.horizontal, self.video_rotation, self.suppress = clip.size, clip.horizontal, clip.video_rotation, False
        self.readout, self.timestamps = float(readout), [timestamp_ms]
        self.tracks, self._nk = clip.tracks, clip.new_k()
        self.sync_offsets, self.duration_ms = (clip.sync_offsets if use_sync_offsets else None), clip.duration_ms
        self._on_lookup = getattr(clip, "on_lookup", None)      # a clip given as plain data may watch its lookups (tests/_tablecase.py counts the ones between unequal keys)

    def time_offset_at(self, k):
        return 0.0

    def new_k(self):
        return self._nk

    def quat_at(self, track, timestamp_ms):
        if self._on_lookup is not None:
            self._on_lookup(track, timestamp_ms, self.sync_offsets, self.duration_ms)
        return H.quat_at(track[0], track[1], timestamp_ms, self.sync_offsets, self.duration_ms)


class Range:
    def __init__(self, clip, pairs, use_sync_offsets=False):
        self.clip, self.use_sync_offsets = clip, use_sync_offsets
        self.pairs = [(int(a), int(b), np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2), np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 2)) for a, b, p, q in pairs]
        self.kp = clip.kernel_params()
        self.kp.lens_correction_amount = 1.0                    # undistort_points_with_rolling_shutter(.., 1.0, false), :63-64

    @property
    def total(self):
        return sum(len(p) for _, _, p, _ in self.pairs)


def side_rotations(rng, ts_us, pts, offs, readout):
    """[n][9] f32, or ONE row when the readout time is zero"""
    timestamp_ms = float(ts_us) / 1000.0 - offs                # `*ts as f64 / 1000.0`, then `timestamp_ms - offs`
    return Z.point_rotations(_Side(rng.clip, timestamp_ms, readout, rng.use_sync_offsets), [(float(x), float(y)) for x, y in pts], 0)


def map_side(rng, ts_us, pts, offs, readout, perturb=None):
    """undistort_points_with_rolling_shutter of one side -> [n][2] f32.  perturb: None or a numpy Generator — the sensitivity measurement of
    _zoomstmt.mapper_for: every entry of every f32 rotation the device derives with its own acos / sin moves by a random -2 .. +2 ULP."""
    if len(pts) == 0:
        return np.zeros((0, 2), dtype=np.float32)
    rot = side_rotations(rng, ts_us, pts, offs, readout)
    if perturb is not None:
        delta = perturb.integers(-2, 3, rot.shape).astype(np.int32)
        rot = np.where(rot == 0.0, rot, (rot.view(np.int32) + delta).view(np.float32))
    if rot.shape[0] == 1:
        rot = np.repeat(rot, len(pts), 0)
    clip = rng.clip
    return O.undistort_points(rng.kp, clip.model, clip.digital, np.ascontiguousarray(rot), points=pts, index_mode=abi.POINT_INDEX_PER_POINT)


def fold(p1, p2, w, h):
    """:66-81 for one pair -> the pair's contribution, a Python int"""
    p1, p2 = np.asarray(p1, dtype=np.float32).reshape(-1, 2), np.asarray(p2, dtype=np.float32).reshape(-1, 2)
    wf, hf = f32(w), f32(h)
    with np.errstate(all="ignore"):
        ok = ((p1[:, 0] > 0.0) & (p1[:, 0] < wf) & (p1[:, 1] > 0.0) & (p1[:, 1] < hf) &
              (p2[:, 0] > 0.0) & (p2[:, 0] < wf) & (p2[:, 1] > 0.0) & (p2[:, 1] < hf))
        a, b = p1[ok], p2[ok]
        dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        dist = (dx * dx) + (dy * dy)                              # float32 arrays: every operation rounds to f32, none fuses
    d = np.sort(dist.astype(np.uint64))                         # `dist as u64`; sort_unstable
    k = int(float(len(d)) * 0.9)
    return int(d[:k].sum(dtype=np.uint64))


def fold_mapped(rng, mapped):
    """calculate_distance's fold over given mapped points [total][2][2] (p1, p2 per point pair) -> f64"""
    w, h = rng.clip.size
    total_dist, at = 0.0, 0
    for _, _, p, _ in rng.pairs:
        m = np.asarray(mapped[at:at + len(p)], dtype=np.float32).reshape(-1, 2, 2)
        total_dist += float(fold(m[:, 0], m[:, 1], w, h))
        at += len(p)
    return total_dist


def mapped_points(rng, offs, readout, perturb=None):
    """p1, p2 of every point pair of the range for one candidate: [total][2][2] f32"""
    out = np.zeros((rng.total, 2, 2), dtype=np.float32)
    at = 0
    for ts, next_ts, p, q in rng.pairs:
        out[at:at + len(p), 0] = map_side(rng, ts, p, offs, readout, perturb)
        out[at:at + len(p), 1] = map_side(rng, next_ts, q, offs, readout, perturb)
        at += len(p)
    return out


def cost(rng, offs, readout, perturb=None):
    """calculate_distance(offs, Some(readout))"""
    return fold_mapped(rng, mapped_points(rng, offs, readout, perturb))


def _as_int(v):
    """`as usize` / `as isize` of a non-negative-or-not f64: truncates, saturates, NaN -> 0 (negative -> 0 for usize; callers of isize pass the sign on)"""
    if v != v:
        return 0
    return int(max(min(v, 2.0 ** 62), -2.0 ** 62))


def coarse_candidates(mode, initial_offset=0.0, search_size=0.0, readout=0.0, fps=30.0):
    """[(offs, readout)] of the first stage: :113-118 (mode 0), :89-95 (mode 1)"""
    if mode == 0:
        return [(initial_offset + (-(search_size / 2.0) + float(i)), readout) for i in range(max(_as_int(search_size), 0))]
    steps = _as_int(1000.0 / fps) if fps else 2 ** 62
    return [(0.0, float(i)) for i in range(-steps, steps)]


def fine_candidates(mode, lowest, readout=0.0):
    """:99-103 / :123-127"""
    vals = [lowest - 1.0 + (float(i) * 0.01) for i in range(FINE)]
    return [(v, readout) for v in vals] if mode == 0 else [(0.0, v) for v in vals]


def find_min(costs):
    """index reduce_with(find_min) returns over candidates in order: `if a.1 < b.1 { a } else { b }` — the last of the minimal ones; None when empty"""
    best = None
    for i, c in enumerate(costs):
        if best is None or not (costs[best] < c):
            best = i
    return best


def search(rng, mode, initial_offset=0.0, search_size=0.0, readout=0.0, fps=30.0):
    """-> None (no candidates), or dict(coarse=[(offs, readout)], coarse_costs, coarse_pick (index), fine, fine_costs, fine_pick, value, cost)"""
    col = 0 if mode == 0 else 1
    coarse = coarse_candidates(mode, initial_offset, search_size, readout, fps)
    if not coarse:
        return None
    cc = [cost(rng, o, r) for o, r in coarse]
    cp = find_min(cc)
    fine = fine_candidates(mode, coarse[cp][col], readout)
    fc = [cost(rng, o, r) for o, r in fine]
    fp = find_min(fc)
    return dict(coarse=coarse, coarse_costs=cc, coarse_pick=cp, fine=fine, fine_costs=fc, fine_pick=fp, value=fine[fp][col], cost=fc[fp])


def find_offsets(rng_of, ranges, mode, initial_offset=0.0, search_size=0.0, readout=0.0, fps=30.0):
    """find_offsets (:10-147) over ranges [(from_us, to_us)]; rng_of(from_us, to_us) -> Range of the pairs whose first timestamp lies inside -> [(timestamp, offset, cost)]"""
    out = []
    for from_ts, to_ts in ranges:
        r = search(rng_of(from_ts, to_ts), mode, initial_offset, search_size, readout, fps)
        if r is None:
            continue
        if mode == 1:
            out.append((0.0, r["value"], r["cost"]))
        elif abs(r["value"] - initial_offset) < search_size * 0.9:                                  # :137
            out.append(((float(from_ts) + float(to_ts - from_ts) / 2.0) / 1000.0, r["value"], r["cost"]))
    return out


# ------------------------------------------------------------------------------------------------ planted ranges
class PlantedClip(Z.Clip):
    """a _zoomstmt.Clip whose smoothing TARGET is constant (the identity), so that both frames of a pair share a world frame and a scene point seen in both maps to
    one output point.  The track a GyroSource stores as "smoothed" is the correction `sq.inverse() * q` (gyro_source/mod.rs:682-684), so for sq = 1 the stored
    smoothed track IS the original one: smoothed(ts) * org(ts)^-1 = 1 and a point's rotation is R(org(its row's time)).  (A constant STORED track would not do: without
    rolling shutter the rotation would be that constant, whatever the offset.)"""

    @property
    def tracks(self):
        org, _ = Z.Clip.tracks.fget(self)
        return org, org


def planted_pairs(clip, offset_ms, readout_ms, n_points, pair_times_ms, seed=5, gap_ms=33.0):
    """Correspondences of a scene seen through the clip's gyro track DELAYED by offset_ms, with the true readout time readout_ms: output-grid points q, then
    p1 = the render's forward map of q (the oracle's undistort_coord over _hoststmt.row_matrices_from_tracks) at ts_A - offset, p2 at ts_B - offset.
    -> (pairs, q per pair).  calculate_distance(offset_ms, readout_ms) maps p1 and p2 back to (nearly) q.

    With rolling shutter the render picks the matrix of the integer row a first guess (the mid-frame matrix) lands in, while the point map takes the time of the
    point's own, fractional, row: under this much motion the two differ by several rows.  The plant follows the model that is searched: the row's time is iterated
    to its fixed point, p = forward(q; one matrix at start_ts + readout / dim * p.y) — for a PlantedClip that matrix is the one of a frame without rolling shutter
    at that time, since smoothed(ts) * org(ts)^-1 = 1."""
    w, h = clip.size
    org, sm = clip.tracks
    nk = np.asarray(clip.new_k(), dtype=np.float64)
    dim = w if clip.horizontal else h
    rolling = abs(readout_ms) > 0.0
    kp = clip.kernel_params()
    kp.lens_correction_amount, kp.matrix_count, kp.canvas_scale = 1.0, 1, 1.0
    kp.flags = (abi.FLAG_HORIZONTAL_RS if clip.horizontal else 0) | (abi.FLAG_HAS_DIGITAL_LENS if clip.digital else 0)
    for i, v in enumerate((0, 0, w, h)):
        kp.source_rect[i] = kp.output_rect[i] = v
    g = np.random.default_rng(seed)

    def forward(ts, x, y):
        """-> (ok, u, v)"""
        start_ts = ts - offset_ms - readout_ms / 2.0
        t_row, uv = ts - offset_ms, (False, 0.0, 0.0)
        for _ in range(8 if rolling else 1):
            m = H.row_matrices_from_tracks(org, sm, nk, t_row, 0.0, 1, dim, video_rotation_deg=clip.video_rotation)
            uv = O.undistort_coord(kp, clip.model, clip.digital, m, float(x), float(y))
            if not (uv[0] and np.isfinite(uv[1]) and np.isfinite(uv[2])):
                return False, 0.0, 0.0
            t_row = start_ts + (readout_ms / float(dim)) * float(uv[1] if clip.horizontal else uv[2])
        return uv
    pairs, qs = [], []
    for n, t in zip(n_points, pair_times_ms):
        q, sides = np.zeros((n, 2), dtype=np.float32), [np.zeros((n, 2), dtype=np.float32), np.zeros((n, 2), dtype=np.float32)]
        i = 0
        while i < n:                                                                # a scene point both frames see: the forward map exists and is finite in both
            x, y = np.float32(g.uniform(0.1 * w, 0.9 * w)), np.float32(g.uniform(0.1 * h, 0.9 * h))
            uv = [forward(ts, x, y) for ts in (t, t + gap_ms)]
            if uv[0][0] and uv[1][0]:
                q[i] = (x, y)
                sides[0][i], sides[1][i] = uv[0][1:], uv[1][1:]
                i += 1
        pairs.append((int(round(t * 1000.0)), int(round((t + gap_ms) * 1000.0)), sides[0], sides[1]))
        qs.append(q)
    return pairs, qs
