"""Host-side mirrors of ``src/core/synchronization/find_offset/``: the "visual features" offset search (visual_features.rs) and, with ``for_rs``,
the rolling-shutter (frame readout time) estimator; the gyro-match offset search (essential_matrix.rs, offset method 0) and the fast initial offset
rs-sync starts from (rs_sync.rs:26-45).

    offsets = synchronization.find_offsets_visual(compute_params, ranges, matched_points, sync_params, backend)

``find_offsets`` (visual_features.rs:10-147) evaluates ``calculate_distance`` for ``search_size`` coarse and 200 fine candidates of every range; here a
range is ONE device call, ``Backend.sync_visual_search`` (gfw_sync_visual_search).  The rotations come from the quaternion tracks the backend holds
(``Backend.set_quaternion_tracks``; with ``for_rs`` also ``set_sync_offsets`` — the offset search clears the offsets, visual_features.rs:13-15).
The 90 %-of-range acceptance rule (:137) and the range's middle timestamp are applied here.

Not covered: clips with per-frame time offsets, stabiliser data or lens meshes, keyframed lens data or video rotation inside a range,
suppress_rotation.  (rs_sync: ``find_offsets_rssync`` below.  The optical flow that produces the matched points: ``optical_flow_pyrlk`` below.)

    offsets = synchronization.find_offsets_essential(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params, backend)
    initial_offset, search_size = synchronization.initial_offset_fast(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params, backend)

``find_offsets`` of essential_matrix.rs:13-91 matches the angular rates pose estimation produced against the gyro's, per range over
``2 * search_size`` coarse and 200 fine candidate offsets; here ALL ranges are one device call, ``Backend.sync_gyro_search`` (gfw_sync_gyro_search).  The guards,
the range cut, the gyro window, the max-angle skip, the two 20 Hz low-pass calls (``warp.lowpass_gyro``), the 90 % rule and the middle timestamp are applied
here.  The estimated rates are the caller's input: ``estimated_gyro`` makes them of the rotations of ``estimate_poses_almeida``.

    poses = synchronization.estimate_poses_almeida(compute_params, pairs, backend, seed=0)
    gyro = synchronization.estimated_gyro({ts_us: pose and pose["euler"]}, fps, lpf, final_pass)

``PoseAlmeida`` (estimate_pose/almeida.rs): one camera rotation per pair of frames from its matched optical-flow points, ALL pairs in one device call,
``Backend.pose_almeida`` (gfw_pose_almeida).  The reference draws its RANSAC rounds from an unseeded generator; here a seed decides them.

    poses = synchronization.estimate_poses_essential(compute_params, pairs, backend, seed=0)
    poses = synchronization.estimate_poses(pose_method, compute_params, pairs, backend, seed=0)

Pose methods 0 (``PoseFindEssentialMat``) and 2 (``PoseEightPoint``, estimate_pose/mod.rs:27-36) both map to ``Backend.pose_essential`` (gfw_pose_essential):
the rotation part of an essential matrix fitted to the pair's undistorted bearings — for pairs whose camera also moved, which Almeida's rotation-only model
does not explain.  Their solvers (OpenCV's findEssentialMat / recoverPose, the arrsac and eight-point crates) are not in the reference tree: neither OpenCV's
LMedS nor ARRSAC is reproduced; what runs is the eight-point scheme in a RANSAC loop that tests/_posessstmt.py states.  ``estimate_poses`` dispatches on the
method as ``EstimatePoseMethod::from`` does (1 and unknown: Almeida); method 3 (``PoseFindHomography``) is not covered.

    matched = synchronization.optical_flow_pyrlk(frames, pairs, features=None, backend=backend)

``OFOpenCVPyrLK::optical_flow_to`` (optical_flow/opencv_pyrlk.rs:63-119): the features of each pair's first frame tracked into its second frame by pyramidal
Lucas-Kanade, ALL pairs in one device call, ``Backend.flow_pyrlk`` (gfw_flow_pyrlk); without features the points are the grid of opencv_dis.rs:62-119.  AKAZE
is not covered.

    matched = synchronization.optical_flow_dis(frames, pairs, backend=backend)

``OFOpenCVDis`` (optical_flow/opencv_dis.rs, the reference's DEFAULT method 2): the DIS dense flow of ALL pairs in one device call, ``Backend.flow_dis``
(gfw_flow_dis), read at the grid points; with its variational refinement: gfw_flow_dis_refined (``variational_iters``).

    features = synchronization.detect_features_pyrlk(frames, backend)

``OFOpenCVPyrLK::detect_features`` (optical_flow/opencv_pyrlk.rs:25-42): the Shi-Tomasi corners of ALL frames in one device call,
``Backend.corners_shi_tomasi`` (gfw_corners_shi_tomasi) — the ``features`` of ``optical_flow_pyrlk``.

    offsets = synchronization.find_offsets_rssync(compute_params, ranges, matched_points, sync_params, backend, track)
    name, cost = synchronization.guess_orientation({name: track}, compute_params, ranges, matched_points, sync_params, backend)
    offsets = synchronization.find_offsets(offset_method, compute_params, ranges, sync_params, backend, ...)

``rs_sync::find_offsets`` (find_offset/rs_sync.rs, offset method 2, the reference's default): ALL ranges in one device call, ``Backend.sync_rs_search``
(gfw_sync_rs_search) — rolling-shutter aware per point, and tolerant of a camera that moved.  The adapter is mirrored here: ``calc_initial_fast`` through
``initial_offset_fast``, ``collect_points``' range cut, ranges under 2 pairs skipped, the readout rules (:74-81), the sign and unit conventions, the
90 %-of-radius rule (:178) and the middle timestamp.  The solver, the ``rs-sync`` crate, is not in the reference tree and is NOT reproduced: what runs is the
search tests/_rssyncstmt.py states.  ``guess_orientation`` is ``guess_orient`` (:190-222) over tracks the caller has already transformed (``apply_transforms``
for the 48 orientations is not covered).  ``find_offsets`` dispatches on the offset method as synchronization/mod.rs:383-388 does.

    optim = synchronization.OptimSync.new(raw_imu)
    points_ms, rank, ratio = optim.run(target_sync_points, trim_ranges_s, backend)

``OptimSync`` (optimsync.rs) decides WHERE in the clip to sync, before any optical flow (lib.rs:2054-2060): ``new`` resamples the gyro at its average rate on
the host (``warp.optim_resample``), ``run`` is ONE device call, ``Backend.sync_optim_points`` (gfw_sync_optim_points) — the windowed spectrum of the whole clip,
band energies, rank, masks, non-maximum suppression and one pick per segment.
"""
import numpy as np

from . import abi
from . import synthetic as S


class SyncParams:
    """The slice of ``SyncParams`` (synchronization/mod.rs) the visual-features search reads: milliseconds."""

    def __init__(self, initial_offset=0.0, search_size=5000.0):
        self.initial_offset, self.search_size = float(initial_offset), float(search_size)


def search_inputs(compute_params, for_rs=False):
    """What gfw_sync_visual_* take for these parameters: (KernelParams, abi.SyncSearch)."""
    cp = compute_params
    w, h = cp.width, cp.height
    fov = 1.0 * w / max(cp.output_width, 1)                                  # get_fov(use_fovs = false), frame_transform.rs:52-58
    nk = S.new_k(cp.lens, fov, cp.output_width, cp.output_height)
    kp = S.base_kernel_params(cp.lens, fov, 1, digital_lens_params=list(cp.digital_lens_params),
                              light_refraction_coefficient=cp.light_refraction_coefficient)      # cpu_undistort.rs:671-683
    kp.width, kp.height, kp.output_width, kp.output_height = w, h, cp.output_width, cp.output_height
    search = abi.SyncSearch(width=w, height=h, horizontal_readout=1 if cp.horizontal_rs else 0, use_sync_offsets=1 if for_rs else 0,
                            video_rotation_deg=float(cp.video_rotation))
    for i, v in enumerate(np.asarray(nk, dtype=np.float64).reshape(9)):
        search.new_k[i] = v
    return kp, search


def find_offsets_visual(compute_params, ranges, matched_points, sync_params, backend, for_rs=False):
    """``find_offsets`` (visual_features.rs:10-147) -> [(timestamp, offset, cost)].

    ``ranges``: [(from_ts_us, to_ts_us)]; ``matched_points``: {ts_us: (next_ts_us, points [n][2], next points [n][2])}, what
    ``get_of_lines_for_timestamp`` returns for the keys of the estimator's sync results — walked in ascending key order, entries whose point sets are empty
    or of different lengths skipped (:36-40)."""
    kp, search = search_inputs(compute_params, for_rs)
    out = []
    for from_ts, to_ts in ranges:
        pairs = []
        for ts in sorted(matched_points):
            if from_ts <= ts < to_ts:
                next_ts, p1, p2 = matched_points[ts]
                if len(p1) and len(p1) == len(p2):
                    pairs.append((ts, next_ts, p1, p2))
        if for_rs:
            r = backend.sync_visual_search(kp, search, pairs, 1, scaled_fps=compute_params.scaled_fps)
            if r.found:
                out.append((0.0, r.value, r.cost))
        else:
            r = backend.sync_visual_search(kp, search, pairs, 0, sync_params.initial_offset, sync_params.search_size, compute_params.frame_readout_time)
            if r.found:
                middle_timestamp = (float(from_ts) + float(to_ts - from_ts) / 2.0) / 1000.0
                if abs(r.value - sync_params.initial_offset) < sync_params.search_size * 0.9:      # :137
                    out.append((middle_timestamp, r.value, r.cost))
    return out


def _max_angle(items):
    """get_max_angle (essential_matrix.rs:93-103)"""
    m = 0.0
    for _, g in items:
        if g is not None:
            for v in g:
                if abs(v) > m:
                    m = abs(v)
    return m


def _lowpassed(freq, sample_rate, items):
    """filter_gyro_forward_backward over [(timestamp_ms, gyro or None)]; the reference ignores the filter's refusal (2 * freq > sample_rate) and goes on unfiltered"""
    from . import warp
    has = np.array([g is not None for _, g in items], dtype=np.uint8)
    xyz = np.array([g if g is not None else (0.0, 0.0, 0.0) for _, g in items], dtype=np.float64).reshape(-1, 3)
    out, _applied = warp.lowpass_gyro(freq, sample_rate, xyz, has)
    rows = np.zeros((len(items), 4), dtype=np.float64)
    rows[:, 0] = [t for t, _ in items]
    rows[:, 1:] = out
    return rows, has


def essential_ranges(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params):
    """The host half of essential_matrix.rs:13-50 -> [(range index, (est [n][4], est_has, gyro [m][4], gyro_has))] for the ranges that reach the search.

    ``estimated_gyro``: {timestamp_us: (timestamp_ms, (x, y, z) or None)} (the estimator's BTreeMap<i64, TimeIMU>); ``raw_imu``: [(timestamp_ms, (x, y, z) or None)]."""
    out = []
    raw_imu_len = len(raw_imu)
    if not estimated_gyro or not (duration_ms > 0.0) or raw_imu_len == 0:                              # :22
        return out
    keys = sorted(estimated_gyro)
    for i, (from_ts, to_ts) in enumerate(ranges):
        if to_ts <= from_ts:                                                                             # :26
            continue
        of_item = [estimated_gyro[k] for k in keys if from_ts <= k < to_ts]                              # range(from_ts..to_ts): the end excluded
        if not of_item:
            continue
        first, last = of_item[0][0], of_item[-1][0]
        gyro_item = [x for x in raw_imu
                     if first - sync_params.search_size <= x[0] + sync_params.initial_offset <= last + sync_params.search_size]      # :31-38
        if _max_angle(of_item) < 3.0:                                                                    # :40-44, on the unfiltered samples
            continue
        sample_rate = float(raw_imu_len) / (duration_ms / 1000.0)
        est, est_has = _lowpassed(20.0, scaled_fps, of_item)
        gyro, gyro_has = _lowpassed(20.0, sample_rate, gyro_item)
        out.append((i, (est, est_has, gyro, gyro_has)))
    return out


def find_offsets_essential(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params, backend):
    """``find_offsets`` (essential_matrix.rs:13-91) -> [(timestamp, offset, cost)]: one ``Backend.sync_gyro_search`` call for all ranges that reach the search."""
    live = essential_ranges(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params)
    if not live:
        return []
    results = backend.sync_gyro_search([r for _, r in live], sync_params.initial_offset, sync_params.search_size)
    out = []
    for (i, _), r in zip(live, results):
        if not r.found:
            continue
        from_ts, to_ts = ranges[i]
        middle_timestamp = (float(from_ts) + float(to_ts - from_ts) / 2.0) / 1000.0                      # :78
        if abs(r.value - sync_params.initial_offset) < sync_params.search_size * 0.9:                    # :81
            out.append((middle_timestamp, r.value, r.cost))
    return out


def median_offset(values):
    """rs_sync.rs:27-35: the middle of the sorted offsets, the mean of the two middle ones for an even count"""
    v = sorted(float(x) for x in values)
    n = len(v)
    return (v[n // 2 - 1] + v[n // 2]) / 2.0 if n % 2 == 0 else v[n // 2]


def initial_offset_fast(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params, backend):
    """rs_sync.rs:26-45 (``calc_initial_fast``): -> (initial_offset, search_size) the rs-sync solver starts from — the median of the gyro-match offsets and
    3000 ms, or the inputs unchanged when nothing was found."""
    if ranges and len(raw_imu) > 0:
        offsets = find_offsets_essential(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params, backend)
        if offsets:
            return median_offset(o for _, o, _ in offsets), 3000.0
    return sync_params.initial_offset, sync_params.search_size


def rs_readout_time_ms(compute_params):
    """rs_sync.rs:74-80: the frame readout time the solver gets, ms (0 -> half a frame; a global shutter -> 0.01)"""
    cp = compute_params
    t = float(getattr(cp, "frame_readout_time", 0.0))
    if t == 0.0:
        t = 1000.0 / cp.scaled_fps / 2.0
    lens = cp.lens
    if (lens.get("global_shutter") if isinstance(lens, dict) else getattr(lens, "global_shutter", False)):
        t = 0.01
    return t


def rs_inputs(compute_params, flow_size, **solver):
    """What gfw_sync_rs_* take for these parameters: (KernelParams, abi.SyncRsCfg); ``solver``: SyncRsCfg fields other than the defaults."""
    kp, almeida = pose_inputs(compute_params, flow_size)
    cfg = abi.SyncRsCfg(video_width=almeida.video_width, video_height=almeida.video_height, flow_width=almeida.flow_width, flow_height=almeida.flow_height,
                        frame_readout_time_ms=rs_readout_time_ms(compute_params), **solver)
    for i in range(9):
        cfg.camera_matrix[i] = almeida.camera_matrix[i]
    return kp, cfg


def rs_collect_points(ranges, matched_points):
    """``collect_points`` (rs_sync.rs:224-241) and the walk of :107-149 -> [(sync point (from_ts, to_ts), [(ts_a, ts_b, points_a, points_b)])] for the ranges
    of at least 2 pairs.  ``matched_points``: {ts_us: (next_ts_us, points [n][2], next points [n][2])} as ``find_offsets_visual`` takes it."""
    out = []
    keys = sorted(matched_points)
    for from_ts, to_ts in ranges:
        pairs = [(ts,) + tuple(matched_points[ts]) for ts in keys if from_ts <= ts < to_ts] if to_ts > from_ts else []
        if len(pairs) < 2:                                                                               # :108
            continue
        assert all(len(a) == len(b) for _, _, a, b in pairs)                                             # :128
        out.append(((pairs[0][0], pairs[-1][1]), pairs))
    return out


def find_offsets_rssync(compute_params, ranges, matched_points, sync_params, backend, track, calc_initial_fast=False, estimated_gyro=None, raw_imu=(),
                        duration_ms=0.0, flow_size=None, **solver):
    """``find_offsets`` (rs_sync.rs:17-49, :153-188) -> [(timestamp, offset, cost)]: one ``Backend.sync_rs_search`` call for all ranges that reach the search.
    ``track``: (ts_us int64 [n], wxyz f64 [n][4]), the gyro's quaternions (:159).  With ``calc_initial_fast`` the search starts from ``initial_offset_fast``
    of ``estimated_gyro`` / ``raw_imu`` / ``duration_ms``."""
    cp = compute_params
    initial_offset, search_size = sync_params.initial_offset, sync_params.search_size
    if calc_initial_fast:
        initial_offset, search_size = initial_offset_fast(estimated_gyro, raw_imu, duration_ms, cp.scaled_fps, ranges, sync_params, backend)
    live = rs_collect_points(ranges, matched_points)
    if not live:
        return []
    kp, cfg = rs_inputs(cp, flow_size or (cp.width, cp.height), **solver)
    presync_radius, initial_delay = search_size, -initial_offset                                         # :165-166
    results = backend.sync_rs_search(kp, cfg, [pairs for _, pairs in live], track[0], track[1], initial_delay / 1000.0, presync_radius / 1000.0)
    frame_readout_time = cfg.frame_readout_time_ms / 1000.0                                              # :81
    out = []
    for ((from_ts, to_ts), _), r in zip(live, results):
        if not r.found:
            continue
        offset = r.value * 1000.0
        if abs(offset - initial_delay) < presync_radius * 0.9:                                           # :178
            out.append((float(from_ts + to_ts) / 2.0 / 1000.0, -offset - (frame_readout_time * 1000.0 / 2.0), r.cost))
    return out


def guess_orientation(tracks, compute_params, ranges, matched_points, sync_params, backend, flow_size=None, **solver):
    """``guess_orient`` (rs_sync.rs:190-222) over ``tracks``: {name: (ts_us, wxyz)} in the caller's order, each already transformed to its orientation —
    per track one round-0 search of every sync point (``pre_sync``), the picks' costs summed; `if a.1 < b.1 { a } else { b }`: of equal sums the LATER name
    wins.  -> (name, total cost), or None without tracks."""
    cp = compute_params
    live = rs_collect_points(ranges, matched_points)
    solver = dict(solver, rounds=1, refine=0)
    kp, cfg = rs_inputs(cp, flow_size or (cp.width, cp.height), **solver)
    best = None
    for name, (ts_us, wxyz) in tracks.items():
        total = 0.0
        if live:
            for r in backend.sync_rs_search(kp, cfg, [pairs for _, pairs in live], ts_us, wxyz, -sync_params.initial_offset / 1000.0, sync_params.search_size / 1000.0):
                total += r.coarse_cost if r.found else 0.0                                               # unwrap_or((0.0, 0.0))
        best = (name, total) if best is None or not (best[1] < total) else best
    return best


def find_offsets(offset_method, compute_params, ranges, sync_params, backend, matched_points=None, track=None, estimated_gyro=None, raw_imu=(), duration_ms=0.0, **kw):
    """``PoseEstimator::find_offsets`` (synchronization/mod.rs:382-389): 0 -> ``find_offsets_essential``, 1 -> ``find_offsets_visual``, 2 ->
    ``find_offsets_rssync``; an unknown method finds nothing."""
    method = int(offset_method)
    if method == 0:
        return find_offsets_essential(estimated_gyro, raw_imu, duration_ms, compute_params.scaled_fps, ranges, sync_params, backend)
    if method == 1:
        return find_offsets_visual(compute_params, ranges, matched_points, sync_params, backend)
    if method == 2:
        return find_offsets_rssync(compute_params, ranges, matched_points, sync_params, backend, track, estimated_gyro=estimated_gyro, raw_imu=raw_imu,
                                   duration_ms=duration_ms, **kw)
    return []


def scaled_axis(rot):
    """``Rotation3::scaled_axis``: the axis (from the skew part, normalised; none when its norm is not above the f64 epsilon) times the angle acos((trace - 1) / 2)"""
    m = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    axis = np.array([m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    norm = float(np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]))
    if not norm > np.finfo(np.float64).eps:
        return np.zeros(3)
    angle = float(np.arccos(min(max((m[0, 0] + m[1, 1] + m[2, 2] - 1.0) / 2.0, -1.0), 1.0)))
    return axis / norm * angle


def optical_flow_pyrlk(frames, pairs, features=None, backend=None, width=None):
    """``OFOpenCVPyrLK::optical_flow_to`` (optical_flow/opencv_pyrlk.rs:63-119) for all frame pairs in ONE device call (``Backend.flow_pyrlk``).  ``frames``: u8
    gray planes [n][height][stride] (``width`` defaults to the stride); ``pairs``: [(first frame, second frame)] indices; ``features``: one [..][2] array of pixel
    positions per frame, or None for the grid points of opencv_dis.rs:62-119 (computed on the device).  Returns one entry per pair: (pts1 f32 [k][2], pts2 f32
    [k][2]) — the tracked points that pass the reference's filter (:88-100), in feature order — or None when fewer than 10 were kept (:107).  The entries are what
    ``estimate_poses_almeida`` takes as its ``pairs``."""
    if backend is None:
        raise ValueError("optical_flow_pyrlk: no backend for the optical flow")
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    r = backend.flow_pyrlk(frames, frames.shape[2] if width is None else width, pairs, features)
    first, a, b = r["pair_first"], r["points_a"], r["points_b"]
    return [(a[first[p]:first[p + 1]], b[first[p]:first[p + 1]]) if first[p + 1] - first[p] >= 10 else None for p in range(len(first) - 1)]


def optical_flow_dis(frames, pairs, backend=None, width=None, finest_scale=2, variational_iters=0):
    """``OFOpenCVDis::optical_flow_to`` (optical_flow/opencv_dis.rs, the reference's default method 2) for all frame pairs in ONE device call
    (``Backend.flow_dis``): the DIS dense flow with the parameters of DISOpticalFlow_PRESET_FAST, read at the grid points of :62-119.  ``variational_iters``: the
    fixed-point iterations of the preset's variational refinement on every level (gfw_flow_dis_refined).  THE REFERENCE'S PRESET IS 5; the default here stays 0,
    the unrefined flow, as before the refinement existed.  ``frames``: u8 gray planes [n][height][stride] (``width`` defaults to the stride); ``pairs``: [(first frame, second frame)]
    indices; ``finest_scale``: 2 as the reference, or 1 for a flow of half the pixel.  Returns one entry per pair: (pts1 f32 [k][2], pts2 f32 [k][2]) — every node
    the grid keeps in the first frame and where the flow takes it, unfiltered as in the reference (:113-117) — or None when fewer than 10 nodes were kept (:126).
    The entries are what ``estimate_poses_almeida`` takes as its ``pairs``."""
    if backend is None:
        raise ValueError("optical_flow_dis: no backend for the optical flow")
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    r = backend.flow_dis(frames, frames.shape[2] if width is None else width, pairs, finest_scale=finest_scale, variational_iters=variational_iters)
    first, a, b = r["pair_first"], r["points_a"], r["points_b"]
    return [(a[first[p]:first[p + 1]], b[first[p]:first[p + 1]]) if first[p + 1] - first[p] >= 10 else None for p in range(len(first) - 1)]


def detect_features_pyrlk(frames, backend=None, width=None):
    """``OFOpenCVPyrLK::detect_features`` (optical_flow/opencv_pyrlk.rs:25-42) for all frames in ONE device call (``Backend.corners_shi_tomasi``) with the
    reference's parameters, good_features_to_track(img, 200, 0.01, 10.0, ..).  ``frames``: u8 gray planes [n][height][stride] (``width`` defaults to the stride).
    Returns one f32 [k][2] array of pixel positions per frame, in pick order: exactly the ``features`` argument of ``optical_flow_pyrlk``."""
    if backend is None:
        raise ValueError("detect_features_pyrlk: no backend for the corner detection")
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    r = backend.corners_shi_tomasi(frames, frames.shape[2] if width is None else width, max_corners=200, quality=0.01, min_distance=10.0)
    first, feats = r["feat_first"], r["features"]
    return [feats[first[f]:first[f + 1]] for f in range(len(first) - 1)]


def pose_inputs(compute_params, flow_size, num_iters=200, num_samples=1000, inlier_angle=0.05):
    """What gfw_pose_almeida takes for these parameters: (KernelParams, abi.PoseAlmeidaCfg).  The camera matrix is the lens profile's at the clip's size
    (get_lens_data_at_timestamp(..).0): one call per lens."""
    cp = compute_params
    kp = S.base_kernel_params(cp.lens, 1.0, 1, digital_lens_params=list(cp.digital_lens_params),
                              light_refraction_coefficient=cp.light_refraction_coefficient)      # undistort_points(.., 1.0, 1.0, ..): cpu_undistort.rs:671-683
    kp.width, kp.height, kp.output_width, kp.output_height = cp.width, cp.height, cp.output_width, cp.output_height
    cfg = abi.PoseAlmeidaCfg(video_width=cp.width, video_height=cp.height, flow_width=int(flow_size[0]), flow_height=int(flow_size[1]),
                             num_iters=int(num_iters), num_samples=int(num_samples), inlier_angle_deg=float(inlier_angle))
    K = (float(kp.f[0]), 0.0, float(kp.c[0]), 0.0, float(kp.f[1]), float(kp.c[1]), 0.0, 0.0, 1.0)
    for i, v in enumerate(K):
        cfg.camera_matrix[i] = v
    return kp, cfg


def estimate_poses_almeida(compute_params, pairs, backend, seed=0, flow_size=None, every_nth_frame=1, num_iters=200, num_samples=1000):
    """``PoseEstimator::process_detected_frames`` (synchronization/mod.rs:110-167) with the Almeida method for all frame pairs in ONE device call
    (``Backend.pose_almeida``).  ``pairs``: one entry per frame pair in order — None (the optical flow found no lines: no rotation, :141) or
    (points_a [n][2], points_b [n][2]) optical-flow pixels of an image of ``flow_size`` (default: the clip's size).  The reference draws a round's points from an
    unseeded generator; here ``seed`` decides them (``warp.pose_draws``).  Returns one entry per pair: None, or dict(rotation f64 [3][3], quat f32 [4] (w, i, j, k),
    euler = scaled_axis(rotation) * (scaled_fps / every_nth_frame), inliers, round)."""
    from . import warp
    cp = compute_params
    live = [i for i, p in enumerate(pairs) if p is not None]
    out = [None] * len(pairs)
    if not live:
        return out
    kp, cfg = pose_inputs(cp, flow_size or (cp.width, cp.height), num_iters, num_samples)
    sets = [pairs[i] for i in live]
    triples, samples = warp.pose_draws(seed, [len(np.asarray(a).reshape(-1, 2)) for a, _ in sets], cfg.num_iters, cfg.num_samples)
    quats, rotations, best = backend.pose_almeida(kp, cfg, sets, triples, samples)
    for k, i in enumerate(live):
        out[i] = dict(rotation=rotations[k], quat=quats[k], euler=tuple(scaled_axis(rotations[k]) * (cp.scaled_fps / float(every_nth_frame))),
                      inliers=int(best[k, 0]), round=int(best[k, 1]))
    return out


def pose_essential_inputs(compute_params, flow_size, num_iters=200, inlier_threshold=1e-6, min_front=10):
    """What gfw_pose_essential takes for these parameters: (KernelParams, abi.PoseEssentialCfg), as ``pose_inputs`` makes them for gfw_pose_almeida."""
    kp, almeida = pose_inputs(compute_params, flow_size, num_iters)
    cfg = abi.PoseEssentialCfg(video_width=almeida.video_width, video_height=almeida.video_height, flow_width=almeida.flow_width, flow_height=almeida.flow_height,
                               num_iters=int(num_iters), inlier_threshold=float(inlier_threshold), min_front=int(min_front))
    for i in range(9):
        cfg.camera_matrix[i] = almeida.camera_matrix[i]
    return kp, cfg


def estimate_poses_essential(compute_params, pairs, backend, seed=0, flow_size=None, every_nth_frame=1, num_iters=200, inlier_threshold=1e-6):
    """``PoseEstimator::process_detected_frames`` (synchronization/mod.rs:110-167) with pose method 0 or 2 for all frame pairs in ONE device call
    (``Backend.pose_essential``).  ``pairs`` as ``estimate_poses_almeida`` takes them; ``seed`` decides the rounds' eight points (``warp.pose_draws_k``).  Returns
    one entry per pair: None (no points, or no rotation found: under 8 points, under 8 inliers, or too few of them in front of both cameras), or
    dict(rotation f64 [3][3], quat f32 [4] (w, i, j, k), euler = scaled_axis(rotation) * (scaled_fps / every_nth_frame), inliers, round, front)."""
    from . import warp
    cp = compute_params
    live = [i for i, p in enumerate(pairs) if p is not None]
    out = [None] * len(pairs)
    if not live:
        return out
    kp, cfg = pose_essential_inputs(cp, flow_size or (cp.width, cp.height), num_iters, inlier_threshold)
    sets = [pairs[i] for i in live]
    octets = warp.pose_draws_k(seed, [len(np.asarray(a).reshape(-1, 2)) for a, _ in sets], cfg.num_iters, 8)
    quats, rotations, _essential, best = backend.pose_essential(kp, cfg, sets, octets)
    for k, i in enumerate(live):
        if best[k, 3]:
            out[i] = dict(rotation=rotations[k], quat=quats[k], euler=tuple(scaled_axis(rotations[k]) * (cp.scaled_fps / float(every_nth_frame))),
                          inliers=int(best[k, 0]), round=int(best[k, 1]), front=int(best[k, 2]))
    return out


def estimate_poses(pose_method, compute_params, pairs, backend, **kw):
    """The pose method of a sync (estimate_pose/mod.rs:27-36): 0 (`PoseFindEssentialMat`) and 2 (`PoseEightPoint`) -> ``estimate_poses_essential``; 1 and every
    unknown value -> ``estimate_poses_almeida``, as `EstimatePoseMethod::from` falls back; 3 (`PoseFindHomography`) is not covered."""
    method = int(pose_method)
    if method == 3:
        raise NotImplementedError("pose method 3 (PoseFindHomography) is not covered")
    if method in (0, 2):
        return estimate_poses_essential(compute_params, pairs, backend, **kw)
    return estimate_poses_almeida(compute_params, pairs, backend, **kw)


def estimated_gyro(results, fps, lpf=0.0, final_pass=False):
    """The host part of ``recalculate_gyro_data`` (synchronization/mod.rs:269-361) -> {timestamp_us: (timestamp_ms, (x, y, z))}, what ``find_offsets_essential``
    takes.  ``results``: {frame timestamp_us: euler (x, y, z) or None} — every analysed frame, also those without a rotation: a sample sits midway to the NEXT
    analysed frame.  ``final_pass`` interpolates a missing rotation linearly between its neighbours that have one; ``lpf`` > 0 (Hz) runs gfw_lowpass_gyro."""
    from . import warp
    keys = sorted(results)
    gyro = {}
    for n, k in enumerate(keys):
        eul = results[k]
        if final_pass and eul is None:
            prev = next((p for p in reversed(keys[:n]) if results[p] is not None), None)
            nxt = next((p for p in keys[n:] if results[p] is not None), None)
            if prev is not None and nxt is not None:
                ratio = float(k - prev) / float(nxt - prev)
                eul = tuple(a + (b - a) * ratio for a, b in zip(results[prev], results[nxt]))
        if eul is None:
            continue
        ts = float(k) / 1000.0
        if n + 1 < len(keys):
            ts += (float(keys[n + 1]) / 1000.0 - ts) / 2.0
        v = ts * 1000.0
        ts_us = int(np.floor(abs(v) + 0.5) * (1.0 if v >= 0.0 else -1.0))                                # f64::round: halves away from zero
        gyro[ts_us] = (ts, (eul[1] * 180.0 / np.pi, eul[0] * 180.0 / np.pi, eul[2] * 180.0 / np.pi))   # x and y swapped, degrees
    if lpf > 0.0 and fps > 0.0 and gyro:
        order = sorted(gyro)
        xyz, _applied = warp.lowpass_gyro(lpf, fps, np.array([gyro[k][1] for k in order], dtype=np.float64))
        for k, row in zip(order, xyz):
            gyro[k] = (gyro[k][0], (float(row[0]), float(row[1]), float(row[2])))
    return gyro


class OptimSync:
    """``OptimSync`` (optimsync.rs:10-226): the gyro series at its average rate, and the choice of a clip's sync points from it."""

    def __init__(self, sample_rate, gyro):
        self.sample_rate, self.gyro = float(sample_rate), np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1))

    @classmethod
    def new(cls, raw_imu):
        """``OptimSync::new`` (:30-66).  ``raw_imu``: [(timestamp_ms, (x, y, z) or None)]; None without samples, as the reference."""
        from . import warp
        if len(raw_imu) == 0:
            return None
        ts = np.array([float(t) for t, _ in raw_imu], dtype=np.float64)
        has = np.array([0 if g is None else 1 for _, g in raw_imu], dtype=np.uint8)
        xyz = np.array([(0.0, 0.0, 0.0) if g is None else tuple(g) for _, g in raw_imu], dtype=np.float64).reshape(-1, 3)
        gyro, rate = warp.optim_resample(ts, xyz, has)
        return cls(rate, gyro)

    def run(self, target_sync_points, trim_ranges_s, backend):
        """``OptimSync::run`` (:68-225) -> (points_ms, rank before the masks, ratio = 16 / sample_rate): one ``Backend.sync_optim_points`` call."""
        return backend.sync_optim_points(self.gyro, self.sample_rate, target_sync_points, trim_ranges_s)
