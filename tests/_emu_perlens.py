"""Host interpreter of the moving-lens flavour of the specialised kernel (GFW_JIT_PERFRAME=2: gfw_undistort_clip_lens) — _emu_perframe.run_frames_pf for a launch
whose frames also carry their own lens (f, c, k[12], r_limit), refraction coefficient and mesh (tests/emu/emu_perlens_driver.inc)."""
import ctypes as C
import re

import numpy as np

import _bake
import _emu as E
import _emu_perframe as EP
from gyroflow_amd import abi, warp


class LensSlot(C.Structure):
    """GfwLensSlot (gfw_frame.h): a frame's lens slot of a moving-lens launch"""
    _fields_ = [("f", C.c_float * 2), ("c", C.c_float * 2), ("k", C.c_float * 12), ("r_limit_sq", C.c_float), ("refraction", C.c_float),
                ("mesh", C.c_void_p), ("mesh_len", C.c_int32), ("pad_", C.c_int32)]


def lens_slot_of(fr, mesh):
    """(`mesh`: the frame's mesh as a contiguous f32 array, or None)"""
    p = fr.planes[0]["params"]
    rl = np.float32(p.r_limit)
    return LensSlot((C.c_float * 2)(*p.f), (C.c_float * 2)(*p.c), (C.c_float * 12)(*p.k), float(rl * rl), p.light_refraction_coefficient,
                    mesh.ctypes.data if mesh is not None else None, mesh.size if mesh is not None else 0, 0)


def library_key(frames, meshes=None, matrices_on_device=0, raw=False):
    """gfw_debug_jit_key_clip_lens: the definition list (dict) and bake header (text) of the kernel the library builds for the first launch of a
    gfw_undistort_clip_lens call over `frames` and `meshes` (None, or one f32 array or None per frame), or None where that launch would take an ahead-of-time
    kernel.  raw=True: (definition list, header) as the library writes them, bytes."""
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
    lens = (C.c_size_t * n)(*[0 if m is None else len(m) for m in meshes]) if meshes is not None else None
    defs, header, name = C.create_string_buffer(4096), C.create_string_buffer(1 << 16), C.create_string_buffer(128)
    rc = lib.gfw_debug_jit_key_clip_lens(n, npl, barr, parr, tarr, frames[0].model, frames[0].digital, marr, frames[0].matrices.shape[0], matrices_on_device,
                                         lens, EP.ARCH, defs, len(defs), header, len(header), name, len(name))
    if rc == 1:
        return None
    assert rc == 0, (rc, lib.gfw_last_error())
    if raw:
        return defs.value, header.value
    return dict(d.split("=", 1) for d in defs.value.decode().split(";")), header.value.decode()


def restated_key(fr0, extras):
    """this file's restatement of the flavour's definition list and bake header (gfw_api_bake.inc jit_build_defs / bake_header, perframe = 2): flavour 1's with
    the exact first pass, and a header that names neither the lens (f, c, k, r_limit_sq) nor translation2d nor the fill flag"""
    p0 = fr0.planes[0]["params"]
    bps, n0, dw, dh, il = E.launch_shape(fr0)
    lean = fr0.model == abi.MODELS["opencv_fisheye"] and (extras & ~2) == 0
    jit_model = 1 if lean else (-2 if extras & (16 | 32) else -1)
    waves = E.jit_waves(n0, p0.matrix_count, jit_model, extras, p0.interpolation, bps, dh)
    if extras & 8 and waves == 8:
        waves = 7                                     # (jit_build_defs: the per-frame flavours' lens-correction body at seven)
    defs = {"GFW_FRAME_KIND": bps, "GFW_FRAME_TAPS": p0.interpolation, "GFW_JIT_WAVES": waves,
            "GFW_JIT_MODEL": jit_model, "GFW_JIT_T": {1: "uint8_t", 2: "uint16_t", 3: "_Float16", 4: "float"}[bps], "GFW_JIT_N0": n0, "GFW_JIT_DW": dw, "GFW_JIT_DH": dh,
            "GFW_JIT_IL": 1 if il else 0, "GFW_JIT_RB": 1, "GFW_JIT_FAST1": 0, "GFW_JIT_PERFRAME": 2}
    header = _bake.bake_header(fr0, rb=1)
    header, n1 = re.subn(r"#define GFW_BK_extras \(0\)", "#define GFW_BK_extras (%d)" % extras, header)
    header, n2 = re.subn(r"#define GFW_BK_digital \(0\)", "#define GFW_BK_digital (%d)" % (fr0.digital if extras & 2 else 0), header)
    header, n3 = re.subn(r"#define GFW_BK_(t2_[01]|fill_bg|f_[01]|c_[01]|k_[0-3]|r_limit_sq) [^\n]*\n", "", header)
    header, n4 = re.subn(r"#define GFW_BK_(p1_[fc]) [^\n]*\n", lambda m: "#define GFW_BK_%s __builtin_bit_cast(float, 0x00000000u)\n" % m.group(1), header)
    assert (n1, n2, n3, n4) == (1, 1, 12, 2), (n1, n2, n3, n4)
    return defs, header


def run_frames_pl(frames, meshes=None, grid=8, lens_of=None, mesh_of=None):
    """One launch of the moving-lens flavour over `frames` (one shape, the same clip constants and feature bits; <= 16) -> [[plane outputs] per frame].
    `meshes`: None, or one f32 array per frame (every frame or none: whether a mesh is present is compiled in).
    The kernel built is the library's own: its definition list and bake header come from gfw_debug_jit_key_clip_lens, and must equal this file's restatement.
    The argument block's own KernelParams carry NaN where the lens is and the shared block no mesh: whatever the kernel reads of the lens, it reads from the slots.
    `lens_of` / `mesh_of`: frame index -> the index of the frame whose lens / mesh fills the slot (the controls of tests/test_emu_clip_lens.py)."""
    fr0 = frames[0]
    p0 = fr0.planes[0]["params"]
    n = len(frames)
    assert E.fused_eligible(fr0), "not a frame the fused kernel serves"
    assert meshes is None or all(m is not None and len(m) for m in meshes)
    extras = E.feature_bits(fr0, meshes[0] if meshes is not None else None)
    assert all(E.feature_bits(fr, meshes[f] if meshes is not None else None) == extras for f, fr in enumerate(frames)), "the frames of one launch share their feature bits"
    defs, header = restated_key(fr0, extras)
    key = library_key(frames, meshes)
    assert key is not None, "the library would launch an ahead-of-time kernel for these frames"
    lib_defs, lib_header = key
    assert lib_defs == {k: str(v) for k, v in defs.items()}, (lib_defs, defs)
    lib_lines = [l for l in lib_header.splitlines() if not l.startswith("#define GFW_P1_RFORM ")]
    assert sorted(lib_lines) == sorted(header.splitlines()), sorted(set(lib_lines) ^ set(header.splitlines()))
    small = n * p0.output_width * p0.output_height < 400000
    lib = C.CDLL(E.build(lib_defs, lib_header, driver="emu_perlens_driver.inc", opt="-O0" if small else "-O1",
                         extra_flags=("-DGFW_JIT=1", "-DGFW_BAKE=1", "-DEMU_VOTES=0", "-DEMU_HW_ULP=0", "-DEMU_AUDIT=0")))
    lib.gfw_emu_launch_pl.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    pints, pfloats = np.zeros(24, np.int32), np.zeros(20, np.float32)
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
    slots = (EP.FramePer * n)(*[EP.slot_of(fr) for fr in frames])
    held = [np.ascontiguousarray(m, dtype=np.float32) for m in meshes] if meshes is not None else [None] * n
    lens_of, mesh_of = lens_of or (lambda f: f), mesh_of or (lambda f: f)
    lslots = (LensSlot * n)()
    for f in range(n):
        s = lens_slot_of(frames[lens_of(f)], held[mesh_of(f)])
        lslots[f] = s
    kp = abi.KernelParams.from_buffer_copy(p0)
    nan = float("nan")
    kp.f[0] = kp.f[1] = kp.c[0] = kp.c[1] = kp.r_limit = kp.light_refraction_coefficient = nan
    for i in range(12):
        kp.k[i] = nan
    com = E.common_for(fr0, p0)
    rc = lib.gfw_emu_launch_pl(n, srcs, dsts, mats, C.cast(C.byref(kp), C.c_void_p), C.cast(C.byref(com), C.c_void_p), grid, pints.ctypes.data, pfloats.ctypes.data,
                               C.cast(slots, C.c_void_p), C.cast(lslots, C.c_void_p))
    assert rc == 0, "gfw_emu_launch_pl -> %d" % rc
    return outs
