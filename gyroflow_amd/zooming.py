"""Host-side mirror of ``src/core/zooming/mod.rs``: the adaptive-zoom fov series of a clip.

    fovs, minimal_fovs = zooming.calculate_fovs(compute_params, timestamps, method, backend)
    compute_params.fovs = fovs
    # ... FrameTransform.at_timestamp per frame, undistort_clip_params: the reference's recompute-then-render sequence

``calculate_fovs`` (mod.rs:35-70) patches the parameters (fov_scale = 1, no fovs, output size = source size), runs
``FovIterative::find_fov`` for every frame — here ONE device call, ``Backend.zoom_fovs`` (gfw_zoom_fovs), or
``Backend.zoom_fovs_stab`` (gfw_zoom_fovs_stab) when the parameters carry per-frame ``camera_stab_data`` or ``mesh_correction`` — and smooths the
series (``warp.zoom_smooth``: static / dynamic / disabled zoom).  The rotations come from the quaternion tracks the backend
holds (``Backend.set_quaternion_tracks`` / ``set_sync_offsets``): they are the clip's, as for the device matrix builder.

Not covered: keyframed zooming speed.
"""
import numpy as np

from . import abi, warp
from . import synthetic as S

GAUSSIAN_FILTER, ENVELOPE_FOLLOWER = 0, 1          # ZoomMethod (mod.rs:16-29)


def search_inputs(compute_params, timestamps):
    """What gfw_zoom_fovs takes for ``timestamps`` = [(frame, timestamp_ms), ...]: (KernelParams, abi.ZoomSearch, ctypes array of abi.ZoomFrame)."""
    cp = compute_params
    w, h = cp.width, cp.height
    fov = 1.0               # get_fov(use_fovs = false) on the patched params (frame_transform.rs:52-58: 1.0 * width / output_width, output = source); this
                            # ComputeParams carries no focal lengths, so focal_length_fov_compensation is 1
    nk = S.new_k(cp.lens, fov, w, h)                                        # get_new_k with output size = source size (mod.rs:47-49)
    kp = S.base_kernel_params(cp.lens, fov, 1, digital_lens_params=list(cp.digital_lens_params),
                              light_refraction_coefficient=cp.light_refraction_coefficient)      # cpu_undistort.rs:671-683
    kp.width, kp.height, kp.output_width, kp.output_height = w, h, w, h
    search = abi.ZoomSearch(width=w, height=h, org_output_width=cp.output_width, org_output_height=cp.output_height,
                            fov_algorithm_margin=float(cp.fov_algorithm_margin),
                            horizontal_readout=1 if cp.horizontal_rs else 0)
    n = len(timestamps)
    frames = (abi.ZoomFrame * n)()
    nkf = np.asarray(nk, dtype=np.float64).reshape(9)
    for k, (_, ts) in enumerate(timestamps):
        f = frames[k]
        f.timestamp_ms, f.per_frame_time_offset_ms, f.frame_readout_time_ms = float(ts), 0.0, float(cp.frame_readout_time)
        for i in range(9):
            f.new_k[i] = nkf[i]
        f.fov, f.video_rotation_deg = fov, float(cp.video_rotation)
        f.zoom_center[0], f.zoom_center[1] = cp.adaptive_zoom_center_offset
        f.lens_correction_amount = float(cp.lens_correction_amount)
    return kp, search, frames


def frame_tables(compute_params, timestamps):
    """camera_stab_data.get(frame) and mesh_correction.get(frame) of every searched frame: ([dict or None] or None, [mesh or None] or None)"""
    def table(src):
        if src is None:
            return None
        return [src[frame] if 0 <= frame < len(src) else None for frame, _ in timestamps]
    return table(getattr(compute_params, "camera_stab_data", None)), table(getattr(compute_params, "mesh_correction", None))


def calculate_fovs(compute_params, timestamps, method, backend):
    """``calculate_fovs`` (zooming/mod.rs:35-70) -> (fovs, minimal_fovs), two float64 arrays of len(timestamps)."""
    if len(timestamps) == 0:
        return np.zeros(0), np.zeros(0)
    kp, search, frames = search_inputs(compute_params, timestamps)
    stabs, meshes = frame_tables(compute_params, timestamps)
    if stabs is None and meshes is None:
        minimal = backend.zoom_fovs(kp, search, frames)
    else:
        minimal = backend.zoom_fovs_stab(kp, search, frames, stabs=stabs, meshes=meshes)
    return warp.zoom_smooth(minimal, compute_params.adaptive_zoom_window, compute_params.scaled_fps, int(method), compute_params.trim_ranges)
