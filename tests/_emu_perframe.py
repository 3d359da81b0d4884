"""Host interpreter of the per-frame flavour of the specialised kernel (GFW_JIT_PERFRAME: gfw_undistort_clip_params) — _emu.run_frames for a launch whose
frames carry their own translation2d, fov, lens_correction_amount, background margin / feather and fill flag (tests/emu/emu_perframe_driver.inc)."""
import ctypes as C
import re

import numpy as np

import _bake
import _emu as E
from gyroflow_amd import abi, warp


class FramePer(C.Structure):
    """GfwFramePer (gfw_frame.h): a frame's slot of a per-frame launch"""
    _fields_ = [("t2", C.c_float * 2), ("fov", C.c_float), ("lens_correction_amount", C.c_float), ("background_margin", C.c_float),
                ("background_margin_feather", C.c_float), ("fill_bg", C.c_int32), ("pad_", C.c_int32)]


def slot_of(fr):
    p = fr.planes[0]["params"]
    return FramePer((C.c_float * 2)(p.translation2d[0], p.translation2d[1]), p.fov, p.lens_correction_amount, p.background_margin,
                    p.background_margin_feather, 1 if p.flags & abi.FLAG_FILL_WITH_BACKGROUND else 0, 0)


def _envelope_table(frames):
    """The first pass's table sized for every frame of the launch (the library's envelope, gfw_undistort_clip_params): the frames' own tables, the widest one"""
    fr0 = frames[0]
    p0 = fr0.planes[0]["params"]
    fisheye = fr0.model == abi.MODELS["opencv_fisheye"]
    extras = E.feature_bits(fr0)
    stretched = any(st > 0.001 and st != 1.0 for st in (p0.input_horizontal_stretch, p0.input_vertical_stretch))
    rform = fr0.model in E.RADIAL_TABLE_MODELS and extras == 0 and not stretched
    best = None
    for fr in frames:
        if rform:
            t = E.p1_table_radial(fr)
        elif fisheye and extras == 0 and not stretched:
            t = E.p1_table(fr.planes[0]["params"], fr.matrices, p0.matrix_count)
        else:
            t = None
        if t is None:
            return None, rform
        if best is None or float(t[1]) > float(best[1]):
            best = t
    return best, rform


def run_frames_pf(frames, grid=8):
    """One launch of the per-frame flavour over `frames` (one shape, one lens and the same clip constants; <= 16) -> [[plane outputs] per frame]."""
    fr0 = frames[0]
    p0 = fr0.planes[0]["params"]
    assert E.fused_eligible(fr0), "not a frame the fused kernel serves"
    extras = E.feature_bits(fr0)
    assert all(E.feature_bits(fr) == extras for fr in frames), "the frames of one launch share their feature bits"
    bps, n0, dw, dh, il = E.launch_shape(fr0)
    fisheye = fr0.model == abi.MODELS["opencv_fisheye"]
    lean = fisheye and (extras & ~2) == 0
    jit_model = 1 if lean else (-2 if extras & (16 | 32) else -1)
    p1, rform = _envelope_table(frames)
    fast1 = p1 is not None
    rb = 4 if fast1 else 1
    defs = {"GFW_FRAME_KIND": bps, "GFW_FRAME_TAPS": p0.interpolation, "GFW_JIT_WAVES": E.jit_waves(n0, p0.matrix_count, jit_model, extras, p0.interpolation, bps, dh),
            "GFW_JIT_MODEL": jit_model, "GFW_JIT_T": {1: "uint8_t", 2: "uint16_t", 3: "_Float16", 4: "float"}[bps], "GFW_JIT_N0": n0, "GFW_JIT_DW": dw, "GFW_JIT_DH": dh,
            "GFW_JIT_IL": 1 if il else 0, "GFW_JIT_RB": rb, "GFW_JIT_FAST1": 1 if fast1 else 0, "GFW_JIT_PERFRAME": 1}
    if rform and fast1:
        defs["GFW_P1_RFORM"] = 1
    header = _bake.bake_header(fr0, rb=rb)
    header, n1 = re.subn(r"#define GFW_BK_extras \(0\)", "#define GFW_BK_extras (%d)" % extras, header)
    header, n2 = re.subn(r"#define GFW_BK_digital \(0\)", "#define GFW_BK_digital (%d)" % (fr0.digital if extras & 2 else 0), header)
    # the per-frame flavour's header names neither translation2d nor the fill flag (gfw_api_bake.inc bake_header, perframe)
    header, n3 = re.subn(r"#define GFW_BK_(t2_[01]|fill_bg) [^\n]*\n", "", header)
    assert n1 == 1 and n2 == 1 and n3 == 3
    small = len(frames) * p0.output_width * p0.output_height < 400000
    lib = C.CDLL(E.build(defs, header, driver="emu_perframe_driver.inc", opt="-O0" if small else "-O1",
                         extra_flags=("-DGFW_JIT=1", "-DGFW_BAKE=1", "-DEMU_VOTES=0", "-DEMU_HW_ULP=0", "-DEMU_AUDIT=0")))
    lib.gfw_emu_launch_pf.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(frames)
    pints, pfloats = np.zeros(24, np.int32), np.zeros(20, np.float32)
    for i, pl in enumerate(fr0.planes):
        q = pl["params"]
        pints[4 * i:4 * i + 4] = (q.stride, pl["out_size"][2], pl["size"][0], pl["size"][1])
        pfloats[5 * i:5 * i + 4] = [np.float32(q.background[c]) * np.float32(q.max_pixel_value) for c in range(4)]
        pfloats[5 * i + 4] = q.pixel_value_limit
    srcs, dsts, mats, keep, outs = (C.c_void_p * (4 * n))(), (C.c_void_p * (4 * n))(), (C.c_void_p * n)(), [], []
    for f, fr in enumerate(frames):
        packed = warp.pack_matrices(fr.matrices)
        keep.append(packed)
        mats[f] = packed.ctypes.data
        planes = []
        for p, pl in enumerate(fr.planes):
            src = np.concatenate([np.ascontiguousarray(pl["src"]), np.zeros(64, np.uint8)])
            dst = pl["dst"].copy()
            keep.append(src)
            planes.append(dst)
            srcs[4 * f + p], dsts[4 * f + p] = src.ctypes.data, dst.ctypes.data
        outs.append(planes)
    slots = (FramePer * n)(*[slot_of(fr) for fr in frames])
    tab = p1[0] if fast1 else np.zeros((2, 2), np.float32)
    com = E.common_for(fr0, p0)
    rc = lib.gfw_emu_launch_pf(n, srcs, dsts, mats, tab.ctypes.data, p1[1] if fast1 else 0.0, p1[2] if fast1 else 0.0, *(p1[3][:3] if fast1 else (0.0, 0.0, 0.0)),
                               C.cast(C.byref(p0), C.c_void_p), C.cast(C.byref(com), C.c_void_p), grid, pints.ctypes.data, pfloats.ctypes.data,
                               p1[4].ctypes.data if fast1 else None, C.cast(slots, C.c_void_p))
    assert rc == 0, "gfw_emu_launch_pf -> %d" % rc
    return outs
