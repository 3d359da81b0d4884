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
    """The first pass's table sized for the frames of the launch (the library's envelope, gfw_undistort_clip_params): the widest of the frames' own tables.  The
    launch has a certified pass when frame 0 has one (the library decides on the frame that opens the launch); a later frame whose own table the host would decline
    still runs under it — its certificate is its own, evaluated by the kernel from its own matrix and zoom centre."""
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
            if fr is fr0:
                return None, rform
            continue
        if best is None or float(t[1]) > float(best[1]):
            best = t
    return best, rform


ARCH = b"gfx950:sramecc+:xnack-"       # (build_jit_cache.ARCH: part of the cache name only)


def library_key(frames, audit=False, matrices_on_device=0, raw=False):
    """gfw_debug_jit_key_clip_params: the definition list (dict) and bake header (text) of the kernel the library builds for the first launch of a
    gfw_undistort_clip_params call over `frames` (host tables: frame 0's own; 2: device-resident tables, the call's envelope), or None where that launch would take
    an ahead-of-time kernel.  raw=True: (definition list, header) as the library writes them, bytes."""
    lib = abi.load_library()
    n, npl = len(frames), len(frames[0].planes)
    bufs, params, mats = [], [], []
    for f, fr in enumerate(frames):                   # any non-null device pointers: the key holds no pointer
        for p, pl in enumerate(fr.planes):
            bufs.append(warp.device_buffers(0x100000 * (p + 1), pl["size"][2] * pl["size"][1], pl["size"], 0x90000000 + 0x100000 * p, pl["out_size"][2] * pl["out_size"][1], pl["out_size"]))
            params.append(pl["params"])
        mats.append(np.ascontiguousarray(fr.matrices, dtype=np.float32))
    barr, parr = (abi.Buffers * len(bufs))(*bufs), (abi.KernelParams * len(params))(*params)
    tarr = (C.c_int * npl)(*[abi.PIXEL_TYPES[pl["pixel_type"]][0] for pl in frames[0].planes])
    marr = (C.c_void_p * n)(*[m.ctypes.data for m in mats])
    defs, header, name = C.create_string_buffer(4096), C.create_string_buffer(1 << 16), C.create_string_buffer(128)
    rc = lib.gfw_debug_jit_key_clip_params(n, npl, barr, parr, tarr, frames[0].model, frames[0].digital, marr, frames[0].matrices.shape[0], matrices_on_device,
                                           1 if audit else 0, ARCH, defs, len(defs), header, len(header), name, len(name))
    if rc == 1:
        return None
    assert rc == 0, (rc, lib.gfw_last_error())
    if raw:
        return defs.value, header.value
    return dict(d.split("=", 1) for d in defs.value.decode().split(";")), header.value.decode()


def run_frames_pf(frames, grid=8, audit=False, table=None):
    """One launch of the per-frame flavour over `frames` (one shape, one lens and the same clip constants; <= 16) -> [[plane outputs] per frame].
    The kernel built is the library's own: its definition list and bake header come from gfw_debug_jit_key_clip_params, and must equal this file's restatement
    of them (the restatement is what the interpreter's arguments are derived from).
    `audit`: the audit build (GFW_JIT_AUDIT=1, what GFW_OPT_KERNEL_VARIANT 3 / 4 launches) -> (outputs, dict of the audit words as _emu.run_frames(audit=True)
    returns them; eps_px is word 6, the largest certificate half-width E of the launch's frames).
    `table`: the first pass's table and range constants to launch with (a p1 tuple of _emu.p1_table) instead of the frames' envelope."""
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
    if table is not None:
        assert p1 is not None, "a table for a launch without a certified first pass"
        p1 = table
    fast1 = p1 is not None
    rb = 4 if fast1 else 1
    waves = E.jit_waves(n0, p0.matrix_count, jit_model, extras, p0.interpolation, bps, dh)
    if extras & 8 and waves == 8:
        waves = 7                                     # (jit_build_defs: the flavour's lens-correction body at seven)
    defs = {"GFW_FRAME_KIND": bps, "GFW_FRAME_TAPS": p0.interpolation, "GFW_JIT_WAVES": waves,
            "GFW_JIT_MODEL": jit_model, "GFW_JIT_T": {1: "uint8_t", 2: "uint16_t", 3: "_Float16", 4: "float"}[bps], "GFW_JIT_N0": n0, "GFW_JIT_DW": dw, "GFW_JIT_DH": dh,
            "GFW_JIT_IL": 1 if il else 0, "GFW_JIT_RB": rb, "GFW_JIT_FAST1": 1 if fast1 else 0, "GFW_JIT_PERFRAME": 1}
    if audit:
        defs["GFW_JIT_AUDIT"] = 1
    header = _bake.bake_header(fr0, rb=rb)
    header, n1 = re.subn(r"#define GFW_BK_extras \(0\)", "#define GFW_BK_extras (%d)" % extras, header)
    header, n2 = re.subn(r"#define GFW_BK_digital \(0\)", "#define GFW_BK_digital (%d)" % (fr0.digital if extras & 2 else 0), header)
    # the per-frame flavour's header names neither translation2d nor the fill flag (gfw_api_bake.inc bake_header, perframe)
    header, n3 = re.subn(r"#define GFW_BK_(t2_[01]|fill_bg) [^\n]*\n", "", header)
    assert n1 == 1 and n2 == 1 and n3 == 3
    if audit:
        header = header.replace("#define GFW_BK_audit ((unsigned long long *)nullptr)", "#define GFW_BK_audit (A.audit)")
    stretched = any(st > 0.001 and st != 1.0 for st in (p0.input_horizontal_stretch, p0.input_vertical_stretch))
    if extras or stretched or not (fisheye or rform):
        # (p1_setup never ran: build_yuv_args leaves the first pass's focal length and centre at zero — the kernel has no first pass to read them in)
        header, n4 = re.subn(r"#define GFW_BK_(p1_[fc]) [^\n]*\n", lambda m: "#define GFW_BK_%s __builtin_bit_cast(float, 0x00000000u)\n" % m.group(1), header)
        assert n4 == 2
    # the library's key for the same launch: the restatement must be it, line for line (GFW_P1_RFORM is the header's: the radial models' table, whether or not
    # the host certifies the launch)
    key = library_key(frames, audit=audit)
    assert key is not None, "the library would launch an ahead-of-time kernel for these frames"
    lib_defs, lib_header = key
    assert lib_defs == {k: str(v) for k, v in defs.items()}, (lib_defs, defs)
    lib_lines = [l for l in lib_header.splitlines() if not l.startswith("#define GFW_P1_RFORM ")]
    assert sorted(lib_lines) == sorted(header.splitlines()), sorted(set(lib_lines) ^ set(header.splitlines()))
    if fast1 or not rform:
        assert "#define GFW_P1_RFORM (%d)" % (1 if rform else 0) in lib_header.splitlines(), (rform, fast1)
    small = len(frames) * p0.output_width * p0.output_height < 400000
    lib = C.CDLL(E.build(lib_defs, lib_header, driver="emu_perframe_driver.inc", opt="-O0" if small else "-O1",
                         extra_flags=("-DGFW_JIT=1", "-DGFW_BAKE=1", "-DEMU_VOTES=0", "-DEMU_HW_ULP=0", "-DEMU_AUDIT=%d" % (1 if audit else 0))))
    lib.gfw_emu_launch_pf.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(frames)
    pints, pfloats = np.zeros(24, np.int32), np.zeros(20, np.float32)       # [16..23]: the declared lengths (audit builds range-check against them)
    for i, pl in enumerate(fr0.planes):
        q = pl["params"]
        pints[4 * i:4 * i + 4] = (q.stride, pl["out_size"][2], pl["size"][0], pl["size"][1])
        pfloats[5 * i:5 * i + 4] = [np.float32(q.background[c]) * np.float32(q.max_pixel_value) for c in range(4)]
        pfloats[5 * i + 4] = q.pixel_value_limit
        pints[16 + 2 * i], pints[16 + 2 * i + 1] = len(pl["src"]), len(pl["dst"])
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
    if audit:
        words = (C.c_ulonglong * 8)()
        lib.gfw_emu_audit(words, 1)
        f32 = lambda w: float(np.array([int(w) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
        return outs, {"certified": int(words[0]), "wrong": int(words[1]), "queued": int(words[2]), "queue_overflow": int(words[3]), "gap_px": f32(words[4]),
                      "out_of_range": int(words[5]), "eps_px": f32(words[6]) if fast1 else None, "eps_word": int(words[6]), "fast1": fast1}
    return outs
