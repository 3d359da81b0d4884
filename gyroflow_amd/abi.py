"""ctypes view of include/gfwarp.h (the C ABI of libgfwarp).

Nothing here computes pixels: it declares the structs/enums of the boundary and
loads the HIP-built shared library.  There is no CPU fallback — if
``libgfwarp.so`` is missing, :func:`load_library` raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgfwarp.so")


class KernelParams(C.Structure):
    """Byte-exact mirror of ``KernelParams`` (stabilization/mod.rs:101-150), 368 B."""
    _pack_ = 4
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32),
        ("output_width", C.c_int32), ("output_height", C.c_int32), ("output_stride", C.c_int32),
        ("matrix_count", C.c_int32), ("interpolation", C.c_int32), ("background_mode", C.c_int32),
        ("flags", C.c_int32), ("bytes_per_pixel", C.c_int32), ("pix_element_count", C.c_int32),
        ("background", C.c_float * 4), ("f", C.c_float * 2), ("c", C.c_float * 2), ("k", C.c_float * 12),
        ("fov", C.c_float), ("r_limit", C.c_float), ("lens_correction_amount", C.c_float),
        ("input_vertical_stretch", C.c_float), ("input_horizontal_stretch", C.c_float),
        ("background_margin", C.c_float), ("background_margin_feather", C.c_float),
        ("canvas_scale", C.c_float), ("input_rotation", C.c_float), ("output_rotation", C.c_float),
        ("translation2d", C.c_float * 2), ("translation3d", C.c_float * 4),
        ("source_rect", C.c_int32 * 4), ("output_rect", C.c_int32 * 4),
        ("digital_lens_params", C.c_float * 16), ("safe_area_rect", C.c_float * 4),
        ("max_pixel_value", C.c_float), ("distortion_model", C.c_int32), ("digital_lens", C.c_int32),
        ("pixel_value_limit", C.c_float), ("light_refraction_coefficient", C.c_float),
        ("plane_index", C.c_int32), ("reserved1", C.c_float), ("reserved2", C.c_float),
        ("ewa_coeffs_p", C.c_float * 4), ("ewa_coeffs_q", C.c_float * 4),
    ]

    def copy(self):
        out = KernelParams()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(KernelParams))
        return out


assert C.sizeof(KernelParams) == 368

# KernelParamsFlags (stabilization/mod.rs:83-99)
FLAG_FIX_COLOR_RANGE = 1
FLAG_HAS_DIGITAL_LENS = 2
FLAG_FILL_WITH_BACKGROUND = 4
FLAG_DRAWING_ENABLED = 8
FLAG_HORIZONTAL_RS = 16
FLAG_HAS_SOURCE_RECT = 32
FLAG_HAS_OUTPUT_RECT = 64
FLAG_FRAMEBUFFER_INVERTED = 128
FLAG_HAS_IBIS_DATA = 256
FLAG_HAS_MESH_DATA = 512
FLAG_HAS_FPD_DATA = 1024
FLAG_ANY_UNDERWATER = 2048

# Interpolation (stabilization/mod.rs:25-34)
INTERP = {"Bilinear": 2, "Bicubic": 4, "Lanczos4": 8, "RobidouxSharp": 10, "Robidoux": 11,
          "Mitchell": 12, "CatmullRom": 13}

# distortion model ids (include/gfwarp.h)
MODELS = {"none": 0, "opencv_fisheye": 1, "opencv_standard": 2, "poly3": 3, "poly5": 4, "ptlens": 5,
          "insta360": 6, "sony": 7, "generic_polynomial": 8, "gopro": 9, "gopro_superview": 10,
          "gopro_hyperview": 11, "gopro_warp": 12, "digital_stretch": 13, "gopro6_superview": 14}

# PixelType implementors (pixel_formats.rs): name -> (id, numpy dtype, element count, default_max_value)
PIXEL_TYPES = {
    "Luma8": (0, "u1", 1, 255.0), "Luma16": (1, "<u2", 1, 65535.0), "RGB8": (2, "u1", 3, 255.0),
    "RGBA8": (3, "u1", 4, 255.0), "BGRA8": (4, "u1", 4, 255.0), "RGB16": (5, "<u2", 3, 65535.0),
    "RGBA16": (6, "<u2", 4, 65535.0), "AYUV16": (7, "<u2", 4, 65535.0), "RGBAf": (8, "<f4", 4, None),
    "RGBAf16": (9, "<f2", 4, None), "R32f": (10, "<f4", 1, None), "UV8": (11, "u1", 2, 255.0),
    "UV16": (12, "<u2", 2, 65535.0),
}

BUF_NONE, BUF_HOST, BUF_HIP_DEVICE = 0, 1, 2


class FrameTiming(C.Structure):
    """``gfw_frame_timing``: inputs of the device-side per-row matrix builder."""
    _fields_ = [("timestamp_ms", C.c_double), ("per_frame_time_offset_ms", C.c_double), ("frame_readout_time_ms", C.c_double),
                ("new_k", C.c_double * 9), ("video_rotation_deg", C.c_double), ("rows", C.c_int32), ("readout_dim", C.c_int32),
                ("framebuffer_inverted", C.c_int32), ("suppress_rotation", C.c_int32)]


class FrameStab(C.Structure):
    """``gfw_frame_stab``: file_metadata.camera_stab_data[frame] (IBIS/OIS splines) for the device matrix builder."""
    _fields_ = [("offset", C.c_double), ("sensor_size", C.c_double * 2), ("crop_area", C.c_double * 4), ("pixel_pitch", C.c_double * 2),
                ("width", C.c_double), ("height", C.c_double), ("ibis_count", C.c_int32), ("ois_count", C.c_int32),
                ("ibis", C.c_void_p), ("ois", C.c_void_p)]


class ZoomFrame(C.Structure):
    """``gfw_zoom_frame``: one frame of the adaptive-zoom FOV search (gfw_zoom_fovs)."""
    _fields_ = [("timestamp_ms", C.c_double), ("per_frame_time_offset_ms", C.c_double), ("frame_readout_time_ms", C.c_double),
                ("new_k", C.c_double * 9), ("fov", C.c_double), ("video_rotation_deg", C.c_double), ("zoom_center", C.c_double * 2),
                ("lens_correction_amount", C.c_double), ("suppress_rotation", C.c_int32), ("reserved", C.c_int32)]


class ZoomSearch(C.Structure):
    """``gfw_zoom_search``: what every frame of a zoom search shares."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("org_output_width", C.c_int32), ("org_output_height", C.c_int32),
                ("fov_algorithm_margin", C.c_float), ("horizontal_readout", C.c_int32)]


class SyncSearch(C.Structure):
    """``gfw_sync_search``: what every candidate of a visual-features sync search shares."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("horizontal_readout", C.c_int32), ("use_sync_offsets", C.c_int32),
                ("new_k", C.c_double * 9), ("video_rotation_deg", C.c_double), ("reserved", C.c_int32 * 2)]


class SyncResult(C.Structure):
    """``gfw_sync_result``: the two-stage search of one range."""
    _fields_ = [("found", C.c_int32), ("n_coarse", C.c_int32), ("coarse_value", C.c_double), ("coarse_cost", C.c_double),
                ("value", C.c_double), ("cost", C.c_double)]


class PoseAlmeidaCfg(C.Structure):
    """``gfw_pose_almeida_cfg``: what every pair of an Almeida pose estimation call shares."""
    _fields_ = [("video_width", C.c_int32), ("video_height", C.c_int32), ("flow_width", C.c_int32), ("flow_height", C.c_int32),
                ("num_iters", C.c_int32), ("num_samples", C.c_int32), ("inlier_angle_deg", C.c_float), ("reserved", C.c_int32),
                ("camera_matrix", C.c_double * 9)]


class PoseEssentialCfg(C.Structure):
    """``gfw_pose_essential_cfg``: what every pair of an essential-matrix pose estimation call shares."""
    _fields_ = [("video_width", C.c_int32), ("video_height", C.c_int32), ("flow_width", C.c_int32), ("flow_height", C.c_int32),
                ("num_iters", C.c_int32), ("min_front", C.c_int32), ("inlier_threshold", C.c_double), ("reserved", C.c_int32 * 2),
                ("camera_matrix", C.c_double * 9)]

    def __init__(self, *a, **kw):
        kw.setdefault("inlier_threshold", 1e-6)
        kw.setdefault("min_front", 10)
        super().__init__(*a, **kw)


class SyncRsCfg(C.Structure):
    """``gfw_sync_rs_cfg``: what every range of an rs-sync offset search shares (the defaults: the solver's as tests/_rssyncstmt.py states it)."""
    _fields_ = [("video_width", C.c_int32), ("video_height", C.c_int32), ("flow_width", C.c_int32), ("flow_height", C.c_int32),
                ("rounds", C.c_int32), ("refine", C.c_int32), ("hypotheses", C.c_int32), ("refits", C.c_int32), ("jacobi_sweeps", C.c_int32),
                ("reserved", C.c_int32 * 3), ("frame_readout_time_ms", C.c_double), ("step_s", C.c_double), ("loss_scale", C.c_double),
                ("camera_matrix", C.c_double * 9)]

    def __init__(self, *a, **kw):
        for k, v in (("rounds", 4), ("refine", 1), ("hypotheses", 16), ("refits", 3), ("jacobi_sweeps", 5), ("step_s", 3.0 / 1000.0), ("loss_scale", 1000.0)):
            kw.setdefault(k, v)
        super().__init__(*a, **kw)


class FlowPyrLKCfg(C.Structure):
    """``gfw_flow_pyrlk_cfg``: what every frame of a pyramidal Lucas-Kanade optical-flow call shares."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("point_mode", C.c_int32), ("reserved", C.c_int32)]


class CornersCfg(C.Structure):
    """``gfw_corners_cfg``: what every frame of a Shi-Tomasi corner-detection call shares."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("max_corners", C.c_int32), ("quality", C.c_float), ("min_distance", C.c_float),
                ("max_workspace_mb", C.c_int32), ("reserved", C.c_int32)]


class FlowDisCfg(C.Structure):
    """``gfw_flow_dis_cfg``: what every frame of a DIS dense optical-flow call shares."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("finest_scale", C.c_int32), ("variational_iters", C.c_int32), ("reserved", C.c_int32)]


class FlowVarrefCfg(C.Structure):
    """``gfw_flow_varref_cfg``: the variational refinement of a gfw_flow_dis_refined call (the defaults: the preset's values to the builder's best knowledge)."""
    _fields_ = [("fixed_point_iters", C.c_int32), ("sor_iters", C.c_int32), ("alpha", C.c_float), ("delta", C.c_float), ("gamma", C.c_float), ("omega", C.c_float),
                ("reserved", C.c_int32 * 2)]


def varref_cfg(fixed_point_iters=5, sor_iters=5, alpha=20.0, delta=5.0, gamma=10.0, omega=1.6):
    return FlowVarrefCfg(fixed_point_iters=int(fixed_point_iters), sor_iters=int(sor_iters), alpha=alpha, delta=delta, gamma=gamma, omega=omega)


CORNERS_MAX, CORNERS_FRAMES_MAX, CORNERS_SIDE_MIN, CORNERS_SIDE_MAX, CORNERS_WORKSPACE_MB = 4096, 4096, 3, 8192, 512      # gfw_corners_shi_tomasi
CORNERS_RING_SLOTS = 2           # staging slots of gfw_corners_shi_tomasi
FLOW_FEATURES_MAX, FLOW_PAIRS_MAX, FLOW_FRAMES_MAX, FLOW_SIDE_MIN, FLOW_SIDE_MAX = 4096, 65535, 4096, 24, 8192      # gfw_flow_pyrlk
FLOW_RING_SLOTS = 2              # staging slots of gfw_flow_pyrlk
DIS_NODES_MAX, DIS_PAIRS_MAX, DIS_FRAMES_MAX, DIS_SIDE_MAX = 4096, 65535, 4096, 8192      # gfw_flow_dis
DIS_RING_SLOTS = 2               # staging slots of gfw_flow_dis and gfw_flow_dis_refined
VARREF_ITERS_MAX, VARREF_PLANES = 64, 17          # gfw_flow_dis_refined: fixed-point / SOR iterations; work-space floats per pixel and pair of the finest level
POSE_PAIR_POINTS_MAX, POSE_PAIRS_MAX, POSE_ROUNDS_MAX = 4096, 65535, 1024      # gfw_pose_almeida, gfw_pose_essential
POSE_DRAWS_K_MAX = 16            # gfw_pose_draws_k: distinct indices of a round
SYNC_FINE_CANDIDATES = 200       # the second stage's candidates
SYNC_PAIR_POINTS_MAX = 4096
SYNC_GYRO_RANGES_MAX, SYNC_GYRO_EST_MAX, SYNC_GYRO_SAMPLES_MAX, SYNC_GYRO_CANDIDATES_MAX = 65535, 65536, 1 << 22, 2000000      # gfw_sync_gyro_*: per call / per range
SYNC_GYRO_RING_SLOTS = 2         # staging slots of gfw_sync_gyro_*: calls an asynchronous context takes before one waits for an earlier copy
SYNC_RS_PAIR_POINTS_MAX, SYNC_RS_PAIRS_MAX, SYNC_RS_RANGES_MAX, SYNC_RS_TRACK_MAX, SYNC_RS_CANDIDATES_MAX, SYNC_RS_ROUNDS_MAX = 4096, 65535, 65535, 1 << 24, 1 << 20, 8      # gfw_sync_rs_*
SYNC_RS_LATER = 17               # candidates of every round of gfw_sync_rs_search behind the first
SYNC_RS_RING_SLOTS = 2           # staging slots of gfw_sync_rs_*
SYNC_OPTIM_FFT_MIN, SYNC_OPTIM_FFT_MAX, SYNC_OPTIM_SAMPLES_MAX, SYNC_OPTIM_TARGET_MAX, SYNC_OPTIM_TRIM_MAX = 16, 8192, 1 << 24, 65535, 1024      # gfw_sync_optim_*
SYNC_OPTIM_RING_SLOTS = 2        # staging slots of gfw_sync_optim_*
FILTER_NOT_APPLIED = 1           # gfw_lowpass_gyro: the reference's from_params would fail; the data is untouched
ZOOM_RECT_POINTS = 120           # points_around_rect(w, h, 31, 31)


class BufferDesc(C.Structure):
    """``BufferDescription`` (gpu/mod.rs:17-24)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32),
        ("has_rect", C.c_int32), ("rect", C.c_int32 * 4),
        ("has_rotation", C.c_int32), ("rotation", C.c_float),
        ("kind", C.c_int32), ("texture_copy", C.c_int32),
        ("data", C.c_void_p), ("len", C.c_size_t),
    ]


class Buffers(C.Structure):
    """``Buffers`` (gpu/mod.rs:25-28)."""
    _fields_ = [("input", BufferDesc), ("output", BufferDesc)]


ERRORS = {
    0: "Ok", -1: "SizeTooSmall", -2: "SizeMismatch", -3: "InvalidStride", -4: "NoStabilizationData",
    -5: "InputBufferEmpty", -6: "OutputBufferEmpty", -7: "UnsupportedBuffer", -8: "BufferSizeMismatch",
    -9: "InvalidArgument", -10: "NoDevice", -11: "HipError", -100: "Unknown",
}

ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP = -9, -10, -11
POINT_INDEX_SINGLE, POINT_INDEX_PER_POINT, POINT_INDEX_PER_ROW, POINT_INDEX_PER_COLUMN = 0, 1, 2, 3
OPT_SYNCHRONOUS, OPT_MATRICES_ON_DEVICE, OPT_KERNEL_VARIANT, OPT_PROFILE, OPT_TUNE_ROWS, OPT_TUNE_GRID, OPT_JIT, OPT_COALESCE_PLANES, OPT_COALESCE_FRAMES = 1, 2, 3, 4, 5, 6, 7, 8, 9
OPT_FRAME_SYNC = 10
CLIP_MAX = 16                    # GFW_CLIP_FRAMES_MAX: frames gfw_undistort_clip puts into one launch

_lib = None


def bind(lib):
    """Declare argtypes/restypes of every symbol in include/gfwarp.h."""
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.gfw_abi_version.restype = i32
    lib.gfw_list_devices.argtypes = [C.c_char_p, sz]; lib.gfw_list_devices.restype = i32
    lib.gfw_set_device.argtypes = [i32]; lib.gfw_set_device.restype = i32
    lib.gfw_get_info.argtypes = [C.c_char_p, sz]; lib.gfw_get_info.restype = i32
    lib.gfw_is_buffer_supported.argtypes = [C.POINTER(Buffers)]; lib.gfw_is_buffer_supported.restype = i32
    lib.gfw_create.argtypes = [C.POINTER(KernelParams), i32, i32, i32, C.POINTER(Buffers), sz]
    lib.gfw_create.restype = vp
    lib.gfw_destroy.argtypes = [vp]; lib.gfw_destroy.restype = None
    lib.gfw_undistort_image.argtypes = [vp, C.POINTER(Buffers), C.POINTER(KernelParams), vp, i32, vp, sz, vp, sz]
    lib.gfw_undistort_image.restype = i32
    lib.gfw_undistort_frame.argtypes = [vp, i32, C.POINTER(Buffers), C.POINTER(KernelParams), C.POINTER(i32), vp, i32, vp, sz]
    lib.gfw_undistort_frame.restype = i32
    lib.gfw_set_option.argtypes = [vp, i32, C.c_int64]; lib.gfw_set_option.restype = i32
    lib.gfw_get_stream.argtypes = [vp]; lib.gfw_get_stream.restype = vp
    lib.gfw_set_stream.argtypes = [vp, vp]; lib.gfw_set_stream.restype = i32
    lib.gfw_synchronize.argtypes = [vp]; lib.gfw_synchronize.restype = i32
    lib.gfw_flush.argtypes = [vp]; lib.gfw_flush.restype = i32
    lib.gfw_import_external_fd.argtypes = [i32, C.c_size_t, C.c_ulonglong, C.POINTER(vp), C.POINTER(vp)]; lib.gfw_import_external_fd.restype = i32
    lib.gfw_release_external.argtypes = [vp]; lib.gfw_release_external.restype = i32
    lib.gfw_last_backend.argtypes = [vp]; lib.gfw_last_backend.restype = C.c_char_p
    lib.gfw_get_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), i32]; lib.gfw_get_profile.restype = i32
    lib.gfw_get_profile_frames.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]; lib.gfw_get_profile_frames.restype = i32
    lib.gfw_undistort_clip.argtypes = [vp, i32, i32, C.POINTER(Buffers), C.POINTER(KernelParams), C.POINTER(i32), C.POINTER(vp), i32]
    lib.gfw_undistort_clip.restype = i32
    lib.gfw_undistort_clip_params.argtypes = [vp, i32, i32, C.POINTER(Buffers), C.POINTER(KernelParams), C.POINTER(i32), C.POINTER(vp), i32]
    lib.gfw_undistort_clip_params.restype = i32
    lib.gfw_undistort_clip_lens.argtypes = [vp, i32, i32, C.POINTER(Buffers), C.POINTER(KernelParams), C.POINTER(i32), C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(sz)]
    lib.gfw_undistort_clip_lens.restype = i32
    lib.gfw_debug_jit_compile.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz]; lib.gfw_debug_jit_compile.restype = C.c_long
    lib.gfw_jit_status.argtypes = [vp, C.POINTER(C.c_double), C.c_char_p, sz]; lib.gfw_jit_status.restype = i32
    lib.gfw_set_quaternion_tracks.argtypes = [vp, vp, vp, i32, vp, vp, i32]; lib.gfw_set_quaternion_tracks.restype = i32
    lib.gfw_build_matrices.argtypes = [vp, C.POINTER(FrameTiming), vp, C.POINTER(vp)]; lib.gfw_build_matrices.restype = i32
    lib.gfw_build_matrices_stab.argtypes = [vp, C.POINTER(FrameTiming), C.POINTER(FrameStab), vp, C.POINTER(vp)]; lib.gfw_build_matrices_stab.restype = i32
    lib.gfw_set_sync_offsets.argtypes = [vp, C.c_double, vp, vp, i32]; lib.gfw_set_sync_offsets.restype = i32
    lib.gfw_build_matrices_batch.argtypes = [vp, C.POINTER(FrameTiming), i32, C.POINTER(vp)]; lib.gfw_build_matrices_batch.restype = i32
    lib.gfw_build_matrices_batch_stab.argtypes = [vp, C.POINTER(FrameTiming), vp, i32, C.POINTER(vp)]; lib.gfw_build_matrices_batch_stab.restype = i32
    lib.gfw_stmap_undistort.argtypes = [vp, C.POINTER(KernelParams), vp, i32, vp, sz, i32, i32, vp, i32]; lib.gfw_stmap_undistort.restype = i32
    lib.gfw_undistort_points.argtypes = [vp, C.POINTER(KernelParams), vp, sz, i32, vp, i32, vp, i32, vp, sz, vp, i32]; lib.gfw_undistort_points.restype = i32
    lib.gfw_zoom_fovs.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(ZoomSearch), vp, i32, vp, vp, vp, i32]; lib.gfw_zoom_fovs.restype = i32
    lib.gfw_zoom_fovs_stab.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(ZoomSearch), vp, i32, vp, vp, vp, vp, vp, vp, i32]; lib.gfw_zoom_fovs_stab.restype = i32
    lib.gfw_zoom_smooth.argtypes = [vp, i32, C.c_double, C.c_double, i32, vp, i32, vp, vp]; lib.gfw_zoom_smooth.restype = i32
    lib.gfw_sync_visual_costs.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(SyncSearch), vp, vp, vp, vp, i32, vp, i32, vp, vp, i32]; lib.gfw_sync_visual_costs.restype = i32
    lib.gfw_sync_visual_search.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(SyncSearch), vp, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp, i32]
    lib.gfw_sync_visual_search.restype = i32
    lib.gfw_lowpass_gyro.argtypes = [C.c_double, C.c_double, vp, vp, i32]; lib.gfw_lowpass_gyro.restype = i32
    lib.gfw_sync_gyro_costs.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, i32]; lib.gfw_sync_gyro_costs.restype = i32
    lib.gfw_sync_gyro_search.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, i32]; lib.gfw_sync_gyro_search.restype = i32
    lib.gfw_optim_tables.argtypes = [i32, vp, vp, vp]; lib.gfw_optim_tables.restype = i32
    lib.gfw_optim_resample.argtypes = [vp, vp, vp, i32, vp, C.c_int64, vp, vp]; lib.gfw_optim_resample.restype = i32
    lib.gfw_sync_optim_rank.argtypes = [vp, vp, C.c_int64, C.c_double, vp, vp, vp, vp, vp, i32]; lib.gfw_sync_optim_rank.restype = i32
    lib.gfw_sync_optim_points.argtypes = [vp, vp, C.c_int64, C.c_double, i32, vp, i32, vp, vp, vp, vp, vp, i32]; lib.gfw_sync_optim_points.restype = i32
    lib.gfw_pose_almeida.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(PoseAlmeidaCfg), vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32]; lib.gfw_pose_almeida.restype = i32
    lib.gfw_pose_draws.argtypes = [C.c_uint64, vp, i32, i32, i32, vp, vp, vp]; lib.gfw_pose_draws.restype = i32
    lib.gfw_pose_essential.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(PoseEssentialCfg), vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32]; lib.gfw_pose_essential.restype = i32
    lib.gfw_sync_rs_costs.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(SyncRsCfg), vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32]; lib.gfw_sync_rs_costs.restype = i32
    lib.gfw_sync_rs_search.argtypes = [vp, C.POINTER(KernelParams), C.POINTER(SyncRsCfg), vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, C.c_double, C.c_double, vp, vp, vp, i32]
    lib.gfw_sync_rs_search.restype = i32
    lib.gfw_pose_draws_k.argtypes = [C.c_uint64, vp, i32, i32, i32, vp]; lib.gfw_pose_draws_k.restype = i32
    lib.gfw_flow_pyrlk.argtypes = [vp, C.POINTER(FlowPyrLKCfg), vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]; lib.gfw_flow_pyrlk.restype = i32
    lib.gfw_flow_dis.argtypes = [vp, C.POINTER(FlowDisCfg), vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32]; lib.gfw_flow_dis.restype = i32
    lib.gfw_flow_dis_refined.argtypes = [vp, C.POINTER(FlowDisCfg), C.POINTER(FlowVarrefCfg), vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32]; lib.gfw_flow_dis_refined.restype = i32
    lib.gfw_corners_shi_tomasi.argtypes = [vp, C.POINTER(CornersCfg), vp, i32, i32, vp, vp, vp, vp, vp, i32]; lib.gfw_corners_shi_tomasi.restype = i32
    lib.gfw_pack_matrices.argtypes = [vp, i32, vp]; lib.gfw_pack_matrices.restype = i32
    lib.gfw_checksum64.argtypes = [vp, vp, sz, vp]; lib.gfw_checksum64.restype = i32
    lib.gfw_set_frame_checksums.argtypes = [vp, vp, sz]; lib.gfw_set_frame_checksums.restype = i32
    lib.gfw_get_audit.argtypes = [vp, C.POINTER(C.c_ulonglong * 8), i32]; lib.gfw_get_audit.restype = i32
    lib.gfw_debug_math.argtypes = [i32, vp, vp, vp, sz]; lib.gfw_debug_math.restype = i32
    lib.gfw_debug_selftest.argtypes = [i32, C.c_ulonglong, C.c_ulonglong]; lib.gfw_debug_selftest.restype = C.c_longlong
    lib.gfw_last_error.restype = C.c_char_p
    lib.gfw_debug_source_id.argtypes = [C.c_char_p, sz]; lib.gfw_debug_source_id.restype = i32
    lib.gfw_debug_paired_launches.argtypes = [vp]; lib.gfw_debug_paired_launches.restype = C.c_longlong
    lib.gfw_debug_frames_per_launch.argtypes = [C.c_ulonglong, C.c_ulonglong, i32]; lib.gfw_debug_frames_per_launch.restype = i32
    lib.gfw_debug_jit_key_clip_params.argtypes = [i32, i32, C.POINTER(Buffers), C.POINTER(KernelParams), C.POINTER(i32), i32, i32, C.POINTER(vp), i32, i32, i32,
                                                  C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, sz]
    lib.gfw_debug_jit_key_clip_params.restype = i32
    lib.gfw_debug_jit_key_clip_lens.argtypes = [i32, i32, C.POINTER(Buffers), C.POINTER(KernelParams), C.POINTER(i32), i32, i32, C.POINTER(vp), i32, i32, C.POINTER(sz),
                                                C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, sz]
    lib.gfw_debug_jit_key_clip_lens.restype = i32
    lib.gfw_pixel_type_info.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_float)]
    lib.gfw_pixel_type_info.restype = i32
    return lib


EXPORTS = ["gfw_abi_version", "gfw_list_devices", "gfw_set_device", "gfw_get_info", "gfw_is_buffer_supported",
           "gfw_create", "gfw_destroy", "gfw_undistort_image", "gfw_undistort_frame", "gfw_set_option",
           "gfw_get_stream", "gfw_set_stream", "gfw_synchronize", "gfw_flush", "gfw_import_external_fd", "gfw_release_external", "gfw_last_backend", "gfw_get_profile", "gfw_last_error", "gfw_debug_math", "gfw_debug_jit_key", "gfw_debug_selftest", "gfw_get_audit", "gfw_pack_matrices", "gfw_checksum64", "gfw_set_frame_checksums", "gfw_set_quaternion_tracks", "gfw_build_matrices", "gfw_build_matrices_stab", "gfw_set_sync_offsets", "gfw_build_matrices_batch", "gfw_stmap_undistort", "gfw_undistort_points",
           "gfw_pixel_type_info", "gfw_undistort_clip", "gfw_undistort_clip_params", "gfw_jit_status", "gfw_get_profile_frames", "gfw_debug_jit_compile", "gfw_debug_source_id", "gfw_debug_p1_radial", "gfw_debug_paired_launches", "gfw_debug_frames_per_launch",
           "gfw_debug_jit_key_clip_params", "gfw_undistort_clip_lens", "gfw_debug_jit_key_clip_lens", "gfw_zoom_fovs", "gfw_zoom_smooth",
           "gfw_build_matrices_batch_stab", "gfw_zoom_fovs_stab", "gfw_sync_visual_costs", "gfw_sync_visual_search",
           "gfw_lowpass_gyro", "gfw_sync_gyro_costs", "gfw_sync_gyro_search",
           "gfw_optim_tables", "gfw_optim_resample", "gfw_sync_optim_rank", "gfw_sync_optim_points",
           "gfw_pose_almeida", "gfw_pose_draws", "gfw_pose_essential", "gfw_pose_draws_k", "gfw_sync_rs_costs", "gfw_sync_rs_search", "gfw_flow_pyrlk", "gfw_corners_shi_tomasi", "gfw_flow_dis", "gfw_flow_dis_refined"]


def load_library(path=None):
    """Load libgfwarp.so (built by ``__graft_entry__.build()``).  Fails loudly when absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("GFW_LIBRARY", "") or LIB_PATH      # GFW_LIBRARY: A/B builds of the library (tools/, benchmarking)
    if not os.path.exists(p):
        raise RuntimeError(
            "libgfwarp.so not found at %s — the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % p)
    lib = bind(C.CDLL(p))
    if path is None:
        _lib = lib
    return lib


def kernel_source_id():
    """identity of the fused kernel's source inside the loaded library (gfw_debug_source_id): what a stored measurement must name to be quoted for it"""
    buf = C.create_string_buffer(128)
    n = load_library().gfw_debug_source_id(buf, len(buf))
    return buf.value.decode() if n > 0 else ""
