"""The per-frame flavour of the specialised kernel (GFW_JIT_PERFRAME, gfw_undistort_clip_params) costs its clips no occupancy and no scratch: compiled on the
host for gfx950 beside the constant-parameter build of the same clip, it has a 0-byte private segment, the same waves per SIMD, and no transcendental result
read by the next instruction."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from gyroflow_amd import abi, synthetic as S
from _kres import KR, ROOT

SCAN = os.path.join(ROOT, "tools", "scan_trans_hazard.py")


def perframe_key(fr):
    """the per-frame flavour's key of a one-frame gfw_undistort_clip_params call on device-resident tables, from the library itself
    (gfw_debug_jit_key_clip_params): one more definition, no translation2d / fill flag literals; the lens-correction body budgeted at eight waves gets seven"""
    import _emu_perframe as EP
    return EP.library_key([fr], matrices_on_device=2, raw=True)


def compile_(lib, defs, header, out):
    log = C.create_string_buffer(1 << 16)
    n = lib.gfw_debug_jit_compile(b"gfx950", defs, header, out.encode(), log, len(log))
    if n == -2:
        pytest.skip("libhiprtc.so not found")
    assert n > 0, log.value.decode()[-3000:]
    (k,) = [k for elf in KR.code_objects(open(out, "rb").read()) for k in KR.kernels_of(elf)]
    return k


@pytest.mark.parametrize("what,fmt,kw", [
    ("C2 4K dynamic zoom", "YUV422P16LE", dict(fov=1.1, base_overrides={"translation2d": (12.5, -7.25)})),
    ("NV12 lens correction", "NV12", dict(fov=1.1, base_overrides={"lens_correction_amount": 0.5})),
    ("margin and feather", "YUV422P16LE", dict(fov=1.2, base_overrides={"background_mode": 3, "background_margin": 0.1, "background_margin_feather": 0.1})),
])
def test_the_per_frame_flavour_keeps_the_constant_builds_resources(tmp_path, what, fmt, kw):
    import build_jit_cache as B
    lib = abi.load_library()
    lib.gfw_debug_jit_compile.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.gfw_debug_jit_compile.restype = C.c_long
    fr = S.SyntheticFrame(fmt, 3840, 2160, seed=5, pixels=False, **kw)
    defs, header, _ = B.key_of(lib, fr)
    const = compile_(lib, defs, header, str(tmp_path / "const.co"))
    out = str(tmp_path / "perframe.co")
    blend = kw["base_overrides"].get("lens_correction_amount", 1.0) < 1.0 and b"GFW_JIT_WAVES=8" in defs
    pf_defs, pf_header = perframe_key(fr)
    assert pf_defs.split(b";") == [d.replace(b"GFW_JIT_WAVES=8", b"GFW_JIT_WAVES=7") if blend else d for d in defs.split(b";")] + [b"GFW_JIT_PERFRAME=1"], (what, pf_defs)
    assert re.findall(rb"#define GFW_BK_(t2_[01]|fill_bg) ", pf_header) == [] and len(re.findall(rb"#define GFW_BK_(?:t2_[01]|fill_bg) ", header)) == 3, what
    pf = compile_(lib, pf_defs, pf_header, out)
    assert const[".private_segment_fixed_size"] == 0 and pf[".private_segment_fixed_size"] == 0, (what, const[".private_segment_fixed_size"], pf[".private_segment_fixed_size"])
    want = min(KR.waves_per_simd(const[".vgpr_count"]), 7 if blend else 8)
    assert KR.waves_per_simd(pf[".vgpr_count"]) >= want, (what, pf[".vgpr_count"], const[".vgpr_count"])
    assert pf[".kernarg_segment_size"] > const[".kernarg_segment_size"] and pf[".kernarg_segment_size"] <= 4096
    r = subprocess.run([sys.executable, SCAN, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 place(s)" in r.stdout, r.stdout[-2000:]
