"""Host-side mirror of ``src/core/synchronization/find_offset/visual_features.rs``: the "visual features" offset search and, with ``for_rs``,
the rolling-shutter (frame readout time) estimator.

    offsets = synchronization.find_offsets_visual(compute_params, ranges, matched_points, sync_params, backend)

``find_offsets`` (visual_features.rs:10-147) evaluates ``calculate_distance`` for ``search_size`` coarse and 200 fine candidates of every range; here a
range is ONE device call, ``Backend.sync_visual_search`` (gfw_sync_visual_search).  The rotations come from the quaternion tracks the backend holds
(``Backend.set_quaternion_tracks``; with ``for_rs`` also ``set_sync_offsets`` — the offset search clears the offsets, visual_features.rs:13-15).
The 90 %-of-range acceptance rule (:137) and the range's middle timestamp are applied here.

Not covered: clips with per-frame time offsets, stabiliser data or lens meshes, keyframed lens data or video rotation inside a range,
suppress_rotation; the optical flow that produces the matched points, pose estimation, rs_sync, essential_matrix, optimsync.
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
