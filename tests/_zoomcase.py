"""TEST INFRASTRUCTURE: the arguments of gfw_zoom_fovs (product and host-interpreted kernel alike) for a statement clip of tests/_zoomstmt.py."""
import numpy as np

from gyroflow_amd import abi
import _zoomstmt as Z


def inputs(clip, given_rotations=False, tile=1):
    """-> (KernelParams, abi.ZoomSearch, ctypes array of abi.ZoomFrame, rotations [n][9] f32 or None); tile: the clip's frames repeated."""
    kp = clip.kernel_params()
    kp.lens_correction_amount, kp.fov = 1.0, 0.0            # gfw_zoom_fovs reads both from the frame descriptors: these must not matter
    search = abi.ZoomSearch(width=clip.size[0], height=clip.size[1], org_output_width=clip.out[0], org_output_height=clip.out[1],
                            fov_algorithm_margin=clip.margin, horizontal_readout=1 if clip.horizontal else 0)
    ts = list(clip.timestamps) * tile
    frames = (abi.ZoomFrame * len(ts))()
    nk = np.asarray(clip.new_k(), dtype=np.float64).reshape(9)
    for k, t in enumerate(ts):
        f = frames[k]
        f.timestamp_ms, f.per_frame_time_offset_ms = t, clip.time_offset_at(k % len(clip.timestamps))
        f.frame_readout_time_ms = 0.0 if given_rotations else clip.readout
        for i in range(9):
            f.new_k[i] = nk[i]
        f.fov, f.video_rotation_deg = clip.fov, clip.video_rotation
        f.zoom_center[0], f.zoom_center[1] = clip.center_at(k % len(clip.timestamps))
        f.lens_correction_amount = clip.lca_at(k % len(clip.timestamps))
        f.suppress_rotation = 1 if clip.suppress else 0
    rot = None
    if given_rotations:
        rot = np.array([Z.frame_rotation(clip, k) for k in range(len(clip.timestamps))] * tile, dtype=np.float32)
    return kp, search, frames, rot


def readout0(clip):
    """the clip without rolling shutter (caller-given rotations are one per frame)"""
    import copy
    c = copy.copy(clip)
    c.readout = 0.0
    return c


def compute_params(clip, fovs=(), fov_scale=1.0, k=0):
    """the clip (with frame k's zoom centre and lens-correction strength) as stabilization.ComputeParams: the tracks and sync offsets of the statement behind
    org_quat_at / smoothed_quat_at"""
    from gyroflow_amd import stabilization as ST
    org, smoothed = clip.tracks
    return ST.ComputeParams(clip.lens, distortion_model=clip.lens["model"], digital_lens=clip.lens.get("digital"), digital_lens_params=clip.digital_params,
                            width=clip.size[0], height=clip.size[1], output_width=clip.out[0], output_height=clip.out[1], fov_scale=fov_scale, fovs=fovs,
                            frame_readout_time=clip.readout, horizontal_rs=clip.horizontal, lens_correction_amount=clip.lca_at(k),
                            light_refraction_coefficient=clip.refraction, adaptive_zoom_center_offset=clip.center_at(k),
                            org_quat_at=lambda t: clip.quat_at(org, t), smoothed_quat_at=lambda t: clip.quat_at(smoothed, t),
                            video_rotation=clip.video_rotation, fov_algorithm_margin=clip.margin)


def frame_transform(clip, k, fov):
    """FrameTransform.at_timestamp of frame k for fovs = [fov]: the frame's time is its timestamp plus its per-frame time offset"""
    from gyroflow_amd import stabilization as ST
    return ST.FrameTransform.at_timestamp(compute_params(clip, fovs=[fov], k=k), clip.timestamps[k] + clip.time_offset_at(k), 0)


def render_frame(clip, k, fov, background, fmt="NV12", pixels=True, seed=5, transform=None):
    """A synthetic.SyntheticFrame of the clip's frame k whose KernelParams and matrices are FrameTransform.at_timestamp's for fovs = [fov]
    (frame_transform.rs:165-350: new_k from the fov, translation2d from the zoom centre), with a uniform `background`."""
    from gyroflow_amd import stabilization as ST, synthetic as S
    t = transform or frame_transform(clip, k, fov)
    kp = t.kernel_params
    fr = S.SyntheticFrame(fmt, clip.size[0], clip.size[1], seed=seed, fov=t.fov, readout_ms=clip.readout, timestamp_ms=clip.timestamps[k], out_size=clip.out, lens=clip.lens,
                          horizontal_rs=clip.horizontal, background_rgba=(background, background, background, 1.0), pixels=pixels,
                          base_overrides={"lens_correction_amount": clip.lca_at(k), "translation2d": (kp.translation2d[0], kp.translation2d[1]),
                                          "digital_lens_params": clip.digital_params, "light_refraction_coefficient": clip.refraction})
    assert fr.matrices.shape == t.matrices.shape and fr.planes[0]["params"].fov == kp.fov
    fr.matrices = t.matrices
    return fr


def background_pixels(clip, k, fov):
    """pixels of the luma plane that show background when the frame is rendered (by the oracle) with this fov: rendered twice, with two background values"""
    import _oracle as O
    from gyroflow_amd import stabilization as ST
    t = frame_transform(clip, k, fov)
    outs = []
    for bg in (0.0, 1.0):
        fr = render_frame(clip, k, fov, bg, transform=t)
        pl = fr.planes[0]
        dst = pl["dst"].copy()
        assert O.undistort_image(pl["src"], pl["size"], dst, pl["out_size"], pl["params"], pl["pixel_type"], fr.model, fr.digital, fr.matrices) == 1
        outs.append(dst)
    return int(np.count_nonzero(outs[0] != outs[1]))
