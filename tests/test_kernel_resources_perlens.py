"""The moving-lens flavour of the specialised kernel (GFW_JIT_PERFRAME=2, gfw_undistort_clip_lens) costs its clips no scratch and no occupancy: compiled on the
host for gfx950 beside the per-frame flavour (GFW_JIT_PERFRAME=1) of the same clip with the exact first pass, it has a 0-byte private segment wherever that build
has one, at least the waves per SIMD jit_build_defs budgets it for, an argument block inside 4 KB, and no transcendental result read by the next instruction."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import pytest

from gyroflow_amd import abi, synthetic as S
from _kres import KR, ROOT

SCAN = os.path.join(ROOT, "tools", "scan_trans_hazard.py")
W, H = 3840, 2160


def compile_(lib, defs, header, out):
    log = C.create_string_buffer(1 << 16)
    n = lib.gfw_debug_jit_compile(b"gfx950", defs, header, out.encode(), log, len(log))
    if n == -2:
        pytest.skip("libhiprtc.so not found")
    assert n > 0, log.value.decode()[-3000:]
    (k,) = [k for elf in KR.code_objects(open(out, "rb").read()) for k in KR.kernels_of(elf)]
    return k


def lit(name, v):
    return b"#define GFW_BK_%s __builtin_bit_cast(float, 0x%08xu)\n" % (name.encode(), struct.unpack("<I", struct.pack("<f", v))[0])


def flavour_1_exact(defs, header, fr):
    """the per-frame flavour of the same clip with the exact first pass: the moving-lens key with GFW_JIT_PERFRAME=1 and the lens of `fr` back as literals"""
    p = fr.planes[0]["params"]
    lens = b"".join([lit("f_%d" % i, p.f[i]) + lit("c_%d" % i, p.c[i]) for i in range(2)] + [lit("k_%d" % i, p.k[i]) for i in range(4)] + [lit("r_limit_sq", p.r_limit * p.r_limit)])
    assert defs.endswith(b"GFW_JIT_PERFRAME=2")
    return defs[:-1] + b"1", header + lens


def zoom_pair(fmt, mesh=False, **base):
    """two 4K frames of a zoom-lens clip (geometry only): f, c and k differ"""
    frames = []
    for f in range(2):
        lens = S.gopro_style_lens(W, H)
        lens["f"] = tuple(v * (1.0 + 0.05 * f) for v in lens["f"])
        lens["c"] = (lens["c"][0] + 3.0 * f, lens["c"][1] - 2.0 * f)
        lens["k"] = [v * (1.0 + 0.1 * f) for v in lens["k"]]
        frames.append(S.SyntheticFrame(fmt, W, H, seed=5 + f, pixels=False, lens=lens, fov=1.1, base_overrides=dict(base, translation2d=(12.5, -7.25))))
    return frames


@pytest.mark.parametrize("what,fmt,mesh,base", [
    ("C2 4K dynamic zoom", "YUV422P16LE", False, {}),
    ("NV12 lens correction", "NV12", False, {"lens_correction_amount": 0.5}),
    ("NV12 mesh per frame", "NV12", True, {}),
])
def test_the_moving_lens_flavour_keeps_the_per_frame_flavours_resources(tmp_path, what, fmt, mesh, base):
    import numpy as np
    import _emu_perlens as EL
    lib = abi.load_library()
    frames = zoom_pair(fmt, **base)
    meshes = [np.zeros(839, np.float32)] * 2 if mesh else None                # (only its presence enters the key)
    defs, header = EL.library_key(frames, meshes, matrices_on_device=2, raw=True)
    d = dict(x.split(b"=", 1) for x in defs.split(b";"))
    assert d[b"GFW_JIT_PERFRAME"] == b"2" and d[b"GFW_JIT_FAST1"] == b"0" and d[b"GFW_JIT_RB"] == b"1", defs
    assert re.findall(rb"#define GFW_BK_(?:t2_[01]|fill_bg|f_[01]|c_[01]|k_[0-3]|r_limit_sq) ", header) == [], what
    assert (int(d[b"GFW_JIT_MODEL"]), b"(32)" in re.search(rb"#define GFW_BK_extras ([^\n]*)", header).group(1)) == ((-2, True) if mesh else (-1 if base else 1, False))
    one = compile_(lib, *flavour_1_exact(defs, header, frames[0]), str(tmp_path / "perframe.co"))
    out = str(tmp_path / "perlens.co")
    two = compile_(lib, defs, header, out)
    print("%s: flavour 1 (exact first pass) %d VGPR %d SGPR %d B scratch; flavour 2 %d VGPR %d SGPR %d B scratch, %d B of arguments, budget %s waves" % (
        what, one[".vgpr_count"], one[".sgpr_count"], one[".private_segment_fixed_size"], two[".vgpr_count"], two[".sgpr_count"], two[".private_segment_fixed_size"],
        two[".kernarg_segment_size"], d[b"GFW_JIT_WAVES"].decode()))
    if one[".private_segment_fixed_size"] == 0:
        assert two[".private_segment_fixed_size"] == 0, (what, two[".private_segment_fixed_size"])
    assert KR.waves_per_simd(two[".vgpr_count"]) >= int(d[b"GFW_JIT_WAVES"]), (what, two[".vgpr_count"], d[b"GFW_JIT_WAVES"])
    assert one[".kernarg_segment_size"] < two[".kernarg_segment_size"] <= 4096, (one[".kernarg_segment_size"], two[".kernarg_segment_size"])
    r = subprocess.run([sys.executable, SCAN, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 place(s)" in r.stdout, r.stdout[-2000:]
