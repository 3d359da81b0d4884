"""The predicated fetch of the pair's second matrix row (GFW_PAIR_ROW) costs the kernels that carry it no occupancy and no scratch: the C2 clip's build, a 4K NV12
clip's (DH == 2: the fetch per line of the lane's two) and the per-frame flavour of C2, compiled on the host for gfx950 from the source the library embeds, keep a
0-byte private segment, at most 64 VGPRs (eight waves per SIMD; the ahead-of-time budget of tests/test_kernel_resources.py is 80) and the scalar registers of eight
workgroups per CU — as the same builds do with the switch off."""
import ctypes as C

import pytest

from gyroflow_amd import abi, synthetic as S
from _kres import KR


def compile_(lib, defs, header, out):
    lib.gfw_debug_jit_compile.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.gfw_debug_jit_compile.restype = C.c_long
    log = C.create_string_buffer(1 << 16)
    n = lib.gfw_debug_jit_compile(b"gfx950", defs, header, out.encode(), log, len(log))
    if n == -2:
        pytest.skip("libhiprtc.so not found")
    assert n > 0, log.value.decode(errors="replace")[-3000:]
    (k,) = [k for k in KR.report(out) if k[".name"] == "gfw_jit_kernel"]
    return k


def keys(what):
    import build_jit_cache as B
    lib = abi.load_library()
    if what == "C2":
        fr = S.SyntheticFrame("YUV422P16LE", 3840, 2160, seed=0x9F10, pixels=False)
    elif what == "NV12":
        fr = S.SyntheticFrame("NV12", 3840, 2160, seed=0x9F10, pixels=False)
    else:
        fr = S.SyntheticFrame("YUV422P16LE", 3840, 2160, seed=5, fov=1.1, base_overrides={"translation2d": (12.5, -7.25)}, pixels=False)
        import _emu_perframe as EP
        return (lib,) + tuple(EP.library_key([fr], matrices_on_device=2, raw=True))
    defs, header, _ = B.key_of(lib, fr)
    return lib, defs, header


@pytest.mark.parametrize("what", ["C2", "NV12", "per-frame C2"])
def test_the_predicated_fetch_keeps_eight_waves_and_no_scratch(tmp_path, what):
    lib, defs, header = keys(what)
    assert b"GFW_JIT_WAVES=8" in defs and b"GFW_JIT_DW=2" in defs and (b"GFW_JIT_DH=2" in defs) == (what == "NV12"), defs
    assert (b"GFW_JIT_PERFRAME=1" in defs) == (what == "per-frame C2")
    got = {}
    for v in (1, 0):
        k = compile_(lib, defs + b";GFW_PAIR_ROW=%d" % v, header, str(tmp_path / ("pair_row_%d.co" % v)))
        got[v] = (k[".vgpr_count"], k[".sgpr_count"], k[".private_segment_fixed_size"], KR.workgroups_per_cu(k))
    vgpr, sgpr, scratch, wgs = got[1]
    assert scratch == 0 and vgpr <= 64 and KR.waves_per_simd(vgpr) == 8, (what, got)
    assert got[0][2] == 0 and got[0][0] <= 64, (what, got)
    assert sgpr <= 80 and wgs == 8 and wgs >= got[0][3], (what, got)                # floor(800 / (80 + 16)) = 8 workgroups per CU by scalar registers, and LDS admits them
