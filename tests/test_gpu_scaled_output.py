"""Renders at another output size than the source's on every path of the fused kernel: libgfwarp against the oracle fed the same parameters, bit for bit.

gyroflow sets the output size independently of the source size (a 4K clip exported at 1080p, a 1080p clip upscaled, 16:9 rendered to 9:16).  In this library
the output size drives much of the hot path on its own: the chroma ratio and the int_products_exact identities that decide whether a frame is fused
(gfw_api_eligibility.inc), the tile counts, the first pass's rho range (the output frame's corners with host matrices; output size x fov / f with
device-resident ones), the lattice that reaches a tile beyond the last OUTPUT pixel while the row it certifies is clamped to the SOURCE rows, the clip launch
cap, the HOST-buffer copy-back of the written region.  The shapes are tests/_shapes.py's, shared with the CPU tier (tests/test_emu_scaled_output.py).  Every
case asserts the backend it expects, so that a silent fall-back to the per-plane kernel cannot pass."""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
from _shapes import CONTROL, FULL_SIZE, FUSED_SHAPES, MODELS, SHAPES, fused_expected, scaled_frame, sizes
from test_gpu_parity import assert_plane_equal
from test_gpu_fullsize import _View

pytestmark = pytest.mark.gpu

FORMATS = ["NV12", "P010LE", "YUV420P", "YUV422P16LE", "YUV444P16LE", "RGBA", "RGBAF32", "GBRAPF32LE"]


def _frame_cases():
    """Every shape x every format (64 cases); sampler, background mode and shutter direction by a fixed rotation that meets every shape and every format
    with each sampler and each background mode, and each shape and format with both shutter directions."""
    cases = []
    for i, name in enumerate(sorted(SHAPES)):
        for j, fmt in enumerate(FORMATS):
            cases.append((name, fmt, (2, 4, 8)[(i + j) % 3], (i + j) % 4, (j + i // 2) % 2 == 1))
    return cases


def compare(ref, got, fr, what):
    for i, (a, b) in enumerate(zip(ref, got)):
        assert_plane_equal(a, b, fr.planes[i]["pixel_type"], "%s, plane %d" % (what, i))


def check_scaled(fr, fused, what):
    """Oracle vs the frame entry point ahead of time (jit = 0) and specialised (jit = 2), the per-plane kernel, and — where the certified first pass served —
    the exact first pass.  `fused`: whether the fused kernel must serve the frame (else the per-plane kernel must, both ways)."""
    ref = O.run_frame(fr)
    compare(ref, warp.run_frame(fr, jit=2), fr, "%s: specialised (%s)" % (what, warp.last_backend()))
    be2 = warp.last_backend()
    compare(ref, warp.run_frame(fr, jit=0), fr, "%s: ahead of time (%s)" % (what, warp.last_backend()))
    be0 = warp.last_backend()
    if not fused:
        assert be0 == be2 == "plane_generic", (what, be0, be2)
        return be0, be2
    assert be2.startswith("yuv_fused") and be2.endswith("_jit"), (what, be2)
    assert be0.startswith("yuv_fused") and not be0.endswith("_jit"), (what, be0)
    compare(ref, warp.run_frame(fr, fused=False), fr, "%s: plane_generic" % what)
    assert warp.last_backend() == "plane_generic"
    if be0.startswith("yuv_fused_p1") or be2.startswith("yuv_fused_p1"):
        compare(ref, warp.run_frame(fr, variant=2), fr, "%s: exact first pass" % what)
        assert warp.last_backend() == "yuv_fused", warp.last_backend()
    return be0, be2


# ---- the frame entry point ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt,interp,bg,hrs", _frame_cases())
def test_frame_at_another_output_size(name, fmt, interp, bg, hrs):
    ov = {"background_mode": bg}
    if bg == 3:
        ov.update(background_margin=0.08, background_margin_feather=0.1)
    fr = scaled_frame(fmt, name, fov_s=1.0 if bg == 0 else 1.3, seed=0x5CA0 + 7 * len(name) + interp, interpolation=interp, horizontal_rs=hrs,
                      base_overrides=ov, background_rgba=(0.25, 0.5, 0.75, 1.0))
    assert fr.planes[0]["params"].matrix_count == (fr.width if hrs else fr.height)         # one matrix per SOURCE row / column
    check_scaled(fr, fused_expected(name, fmt), "%s %s interp %d bg %d %s" % (name, fmt, interp, bg, "hrs" if hrs else "vrs"))


# ---- clip launches on the certified first pass, device-resident tables ------------------------------------------------------------------------------------
def device_tables_certified(fr):
    """Whether the host certifies the first pass of a frame whose matrices are device-resident (gfw_api_certificate.inc p1_setup): with no host view of the
    geometry it bounds the rho range from the OUTPUT size x fov / f plus 15 degrees of rotation, and a radial model's table over r must be derivable up to
    sqrt(range) x 1.08 (gfw_debug_p1_radial: the library's own derivation).  The 9:16 output's far vertical rays take that range to r = 6.2, where the GoPro
    model's Newton inversion is not certified: those frames take the exact first pass (and must still equal the oracle); every other shape and model is served."""
    import ctypes as C
    import math
    if fr.lens["model"] == "opencv_fisheye":
        return True
    p0 = fr.planes[0]["params"]
    hx, hy = 0.5 * p0.output_width * p0.fov / abs(p0.f[0]), 0.5 * p0.output_height * p0.fov / abs(p0.f[1])
    ang = math.atan(math.hypot(hx, hy)) + 0.26
    rho = min(math.tan(ang) ** 2, 64.0) if ang < 1.45 else 64.0
    lib = abi.load_library()
    lib.gfw_debug_p1_radial.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    tab, out = np.zeros((8193, 2), np.float32), np.zeros(7, np.float64)
    return lib.gfw_debug_p1_radial(C.byref(p0), fr.model, min(math.sqrt(rho) * 1.08, 8.0), tab.ctypes.data, out.ctypes.data) == 1


def test_only_the_portrait_gopro_range_is_declined_on_device_tables():
    """(The expectation the clip and audit cases below draw from device_tables_certified, pinned: one shape x model pair is declined, not a silent many.)"""
    declined = [(n, m) for n in sorted(SHAPES) for m in MODELS if not device_tables_certified(scaled_frame("YUV422P16LE", n, model=m, pixels=False))]
    assert declined == [("portrait", "gopro")], declined


def _check_clip(frames, what):
    import test_gpu_jit as J
    backend, status, (ms, launches, covered), outs, srcs = J.device_clip(frames, 2, True)
    expect = "yuv_fused_p1_jit" if device_tables_certified(frames[0]) else "yuv_fused_jit"
    assert backend == expect and status[0] == 2 and launches == 1 and covered == len(frames), (what, backend, status, launches, covered)
    for j, fr in enumerate(frames):
        compare(O.run_frame(_View(fr, srcs[j])), outs[j], fr, "%s clip launch, frame %d" % (what, j))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FUSED_SHAPES)
def test_clip_launch_on_the_certified_pass(name, model):
    i = FUSED_SHAPES.index(name) + MODELS.index(model)
    fmt, n = ("YUV422P16LE", "NV12")[i % 2], 3 + i % 3
    frames = [scaled_frame(fmt, name, model=model, seed=0x5C10 + j, timestamp_ms=1000.0 + 33.3 * j, pixels=False) for j in range(n)]
    _check_clip(frames, "%s %s %s" % (name, model, fmt))


@pytest.mark.parametrize("name", sorted(FULL_SIZE))
def test_full_size_clip_launch_on_the_certified_pass(name):
    frames = [scaled_frame("YUV422P16LE", name, seed=0x5C20 + j, timestamp_ms=1000.0 + 33.3 * j, pixels=False) for j in range(3)]
    _check_clip(frames, name)


_CAP_SCRIPT = r"""
import sys, json
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import _oracle as O
import test_gpu_jit as J
from _shapes import scaled_frame
frames = [scaled_frame("YUV422P16LE", %(name)r, seed=0x5C30 + j, timestamp_ms=1000.0 + 33.3 * j, pixels=False) for j in range(%(n)d)]
backend, status, (ms, launches, covered), outs, srcs = J.device_clip(frames, 2, True)
bad = 0
for j, fr in enumerate(frames):
    for a, b in zip(O.run_frame(J._View(fr, srcs[j])), outs[j]):
        bad += int(np.count_nonzero(np.asarray(a) != np.asarray(b)))
print("RESULT " + json.dumps({"backend": backend, "launches": int(launches), "covered": int(covered), "bad": bad}))
"""


@pytest.mark.parametrize("name,mb,n", [("up_double", 3, 5), ("down_half", 5, 6)])
def test_the_clip_launch_cap_counts_the_output_planes(tmp_path, name, mb, n):
    """gfw_api_clip.inc clip_launch_limit caps a launch at GFW_CLIP_LAUNCH_MB of source + destination.  The destination is the OUTPUT planes: it used to be
    counted over the source rows (dst stride x input height), which under-counts an upscaled render (320x180 -> 640x360 4:2:2 16-bit: 0.83 MB per frame
    instead of 1.34, three frames to a 3 MB launch instead of two) and over-counts a downscaled one (768x432 -> 384x216: 2.10 MB instead of 1.71).  The cap
    is read once per process: its own interpreter."""
    import json, os, subprocess, sys
    fr = scaled_frame("YUV422P16LE", name, pixels=False)
    per_frame = sum(pl["size"][2] * pl["size"][1] + pl["out_size"][2] * pl["out_size"][1] for pl in fr.planes)
    cap = min(max((mb << 20) // per_frame, 2), abi.CLIP_MAX)
    want = -(-n // cap)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "cap.py"
    script.write_text(_CAP_SCRIPT % {"root": root, "tests": os.path.join(root, "tests"), "name": name, "n": n})
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GFW_CLIP_LAUNCH_MB=str(mb)), capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and line, (r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(line[-1][7:])
    assert res["backend"] == "yuv_fused_p1_jit" and res["covered"] == n and res["bad"] == 0, res
    assert res["launches"] == want, (res, per_frame, cap, want)


# ---- certificate audits -----------------------------------------------------------------------------------------------------------------------------------
def audit_device_tables(fr, variant):
    """The audit instantiation with the frame's planes and its matrix table on the device (GFW_OPT_MATRICES_ON_DEVICE = 2: the host bounds the rho range from
    output size x fov / f alone).  -> (backend, audit words, [output planes])."""
    import torch
    dev = torch.device("cuda", 0)
    src, dst = fr.device_planes(dev), fr.device_outputs(dev)
    d_mat = torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev)
    torch.cuda.synchronize(dev)
    bufs = [warp.device_buffers(s.data_ptr(), s.numel(), pl["size"], d.data_ptr(), d.numel(), pl["out_size"]) for s, d, pl in zip(src, dst, fr.planes)]
    params, types = [pl["params"] for pl in fr.planes], [pl["pixel_type"] for pl in fr.planes]
    be = warp.Backend(params[0], types[0], fr.model, fr.digital, bufs[0])
    try:
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        be.set_option(abi.OPT_KERNEL_VARIANT, variant)
        be.get_audit(reset=True)
        warp.FrameCall(be, bufs, params, types, d_mat.data_ptr(), fr.matrices.shape[0])()
        be.synchronize()
        backend, a = warp.last_backend(), be.get_audit_full()
    finally:
        be.close()
    torch.cuda.synchronize(dev)
    return backend, a, [t.cpu().numpy() for t in dst]


def check_audit(a, pixels, what):
    assert a["certified1_wrong"] == 0 and a["out_of_range"] == 0, (what, a)
    assert a["certified1"] + a["queued1"] + a["queue_overflow"] == pixels, (what, a)
    assert a["pass1_eps_px"] > 0.0 and a["pass1_gap_px"] < a["pass1_eps_px"], (what, a)
    assert a["certified1"] > 0, (what, a)


@pytest.mark.parametrize("variant", [3, 4])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", sorted(SHAPES) + sorted(CONTROL))
def test_certificates_at_another_output_size(name, model, variant):
    """GFW_OPT_KERNEL_VARIANT 3 (the lattice form of the fisheye's first pass) and 4 (the per-pixel form), host and device-resident matrices: the audit build
    re-derives the exact row of every certified pixel.  (An odd output is fused only without subsampled chroma: 4:4:4 there.)"""
    import test_gpu_pass1_radial as R
    fmt = "YUV444P16LE" if name == "odd_out" else "YUV422P16LE"
    fr = scaled_frame(fmt, name, model=model, seed=0xA0D0 + variant, readout_ms=14.0)
    ow, oh = sizes(name)[1]
    expect = "yuv_fused_p1" if model == "opencv_fisheye" else "yuv_fused_p1_jit"         # (the audit of a table over r is a specialised build: gfw_api_bake.inc)
    ref = O.run_frame(fr)
    for kind in ("host", "device"):
        what = "%s %s variant %d, %s matrices" % (name, model, variant, kind)
        backend, a, outs = R.audit(fr, variant) if kind == "host" else audit_device_tables(fr, variant)
        if kind == "device" and not device_tables_certified(fr):
            assert backend == "yuv_fused", (what, backend)                              # declined by the host: the exact first pass, still bit-exact
            compare(ref, outs, fr, what)
            continue
        assert backend == expect, (what, backend)
        check_audit(a, ow * oh, what)
        print("%s: certified %.4f, gap / E %.3f" % (what, a["certified1"] / float(ow * oh), a["pass1_gap_px"] / a["pass1_eps_px"]))
        compare(ref, outs, fr, what)


SWEEP_FAMILIES = ["same"] + FUSED_SHAPES                   # "same": output = input, the control


def random_scaled_clip(rng):
    """A random clip as tests/test_gpu_pass1_sweep.py random_clip draws it (fisheye lens, field of view 0.5-3, rotation up to 15 degrees per axis, readout
    +-30 ms at up to 250 deg/s, both shutter directions) at a random (input, output) pair of a shape family, the output 1x-10x the family's, up to 4K."""
    fam = SWEEP_FAMILIES[int(rng.integers(0, len(SWEEP_FAMILIES)))]
    (iw0, ih0), (ow0, oh0) = SHAPES["down_half" if fam == "same" else fam]
    scale = [1.0, 2.5, 5.0, 10.0][int(rng.integers(0, 4))]
    ow, oh = int(round(ow0 * scale / 2)) * 2, int(round(oh0 * scale / 2)) * 2
    w, h = (ow, oh) if fam == "same" else (int(round(ow * iw0 / ow0 / 2)) * 2, int(round(oh * ih0 / oh0 / 2)) * 2)
    lens = S.gopro_style_lens(w, h)
    f = rng.uniform(0.3, 1.2) * w
    lens["f"] = (f, f * rng.uniform(0.98, 1.02))
    lens["c"] = (w * rng.uniform(0.45, 0.55), h * rng.uniform(0.45, 0.55))
    lens["k"] = [rng.uniform(-0.05, 0.3), rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02)] + [0.0] * 8
    fov = rng.uniform(0.5, 3.0) * w / ow                                            # get_fov: the source's field of view over the output
    hrs = bool(rng.integers(0, 4) == 0)
    readout = rng.uniform(-30.0, 30.0)
    if abs(readout) < 0.5:
        readout = 8.0
    fr = S.SyntheticFrame("YUV422P16LE" if rng.integers(0, 2) else "NV12", w, h, seed=int(rng.integers(1, 1 << 30)), lens=lens, fov=fov,
                          out_size=(ow, oh), readout_ms=readout, horizontal_rs=hrs, pixels=False)
    from test_gpu_pass1_sweep import rot
    rows = fr.matrices.shape[0]
    base = np.radians(rng.uniform(-15.0, 15.0, 3))
    rate = np.radians(rng.uniform(-250.0, 250.0, 3)) * (readout / 1000.0)
    nk = S.new_k(lens, fov, ow, oh)                                                 # the new camera is centred on the OUTPUT
    t = (np.arange(rows) / max(rows - 1, 1)) - 0.5
    m = np.zeros((rows, 14), dtype=np.float32)
    for y in range(rows):
        r = rot(*(base + rate * t[y]))
        r[0, 1] *= -1.0; r[0, 2] *= -1.0; r[1, 0] *= -1.0; r[2, 0] *= -1.0
        m[y, :9] = np.linalg.inv(nk @ r).reshape(9).astype(np.float32)
    fr.matrices = m
    return fam, fr


def test_sixty_random_scaled_clips_never_produce_a_wrong_certificate():
    from test_gpu_pass1_sweep import audit_device
    rng = np.random.default_rng(0x5CA1)
    stats = {fam: [0, 0, 0, 0, 0.0] for fam in SWEEP_FAMILIES}          # clips, served, pixels, certified, worst gap / E
    for i in range(60):
        fam, fr = random_scaled_clip(rng)
        ow, oh = fr.out_size
        backend, a = audit_device(fr)
        st = stats[fam]
        st[0] += 1
        if backend != "yuv_fused_p1":                       # the host declined the certified pass (ray range beyond the table, E too wide): exact first pass
            assert backend == "yuv_fused", (i, fam, backend)
            continue
        what = "clip %d (%s, %dx%d -> %dx%d)" % (i, fam, fr.width, fr.height, ow, oh)
        assert a["certified1_wrong"] == 0 and a["out_of_range"] == 0, (what, a)
        assert a["certified1"] + a["queued1"] + a["queue_overflow"] == ow * oh, (what, a)
        assert a["pass1_eps_px"] > 0.0 and a["pass1_gap_px"] < a["pass1_eps_px"], (what, a)
        st[1] += 1
        st[2] += ow * oh
        st[3] += a["certified1"]
        st[4] = max(st[4], a["pass1_gap_px"] / a["pass1_eps_px"])
    for fam in SWEEP_FAMILIES:
        c, s, p, k, g = stats[fam]
        print("%-20s %2d clips, %2d served, %5.1f %% of their pixels certified, worst gap / E %.3f" % (fam, c, s, 100.0 * k / max(p, 1), g))
    served = sum(st[1] for st in stats.values())
    print("served %d of 60" % served)
    assert served >= 40, served            # (48 of 60 on the MI355X: the declined ones are wide fields of view whose range leaves the table, as in the out = in sweep)


# ---- the render loop's call sequence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["down_half", "up_double"])
@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12"])
def test_render_loop_holds_frames_for_a_clip_launch(name, fmt):
    """One context per plane, GFW_OPT_COALESCE_FRAMES = 4: the per-plane calls of six frames leave as two launches (4 + 2) of the specialised kernel."""
    from test_gpu_coalesce import PlaneLoop
    n = 6
    loop = PlaneLoop([scaled_frame(fmt, name, seed=0xC0A1 + j, timestamp_ms=1000.0 + 33.3 * j) for j in range(n)], jit=2, frames_per_launch=4)
    try:
        loop.be[0].set_option(abi.OPT_PROFILE, 1)            # (the owner context, plane 0, launches every frame)
        backends = []
        for j in range(n):
            loop.frame(j)
            backends.append(warp.Backend.last_backend_of(loop.be[0]))
        for be in loop.be:
            be.synchronize()
        _, launches, covered = loop.be[0].get_profile_frames()
        assert loop.be[0].jit_status()[0] == 2
        assert all(b.startswith("yuv_fused") and b.endswith("_jit") for b in backends), backends
        assert (launches, covered) == (2, n), (launches, covered)
        for j in range(n):
            loop.check(j, "%s %s render loop" % (name, fmt))
    finally:
        loop.close()


# ---- HOST buffers whose written region is smaller than the buffer -----------------------------------------------------------------------------------------
def assert_outside_untouched(fr, got, sentinel=0x5A):
    """Every byte of each output buffer outside its output rect (the whole plane when there is none) still holds the sentinel."""
    for i, (pl, b) in enumerate(zip(fr.planes, got)):
        p = pl["params"]
        obw, obh, ostride = pl["out_size"]
        bpp = p.bytes_per_pixel
        x0, y0, rw, rh = (p.output_rect[k] for k in range(4))
        inside = np.zeros((obh, ostride), dtype=bool)
        inside[y0:y0 + rh, x0 * bpp:(x0 + rw) * bpp] = True
        b2 = b.reshape(obh, ostride)
        assert np.all(b2[~inside] == sentinel), "plane %d: %d bytes outside the written region changed" % (i, int(np.count_nonzero(b2[~inside] != sentinel)))
        assert np.any(b2[inside] != sentinel), "plane %d: nothing written" % i


@pytest.mark.parametrize("name", ["down_half", "up_double"])
@pytest.mark.parametrize("fmt,interp,jit", [("YUV422P16LE", 2, 0), ("NV12", 4, 2), ("YUV420P", 2, 2), ("RGBA", 8, 0), ("RGBAF32", 2, 2)])
def test_output_window_of_a_larger_host_surface(name, fmt, interp, jit):
    from test_gpu_fused_coverage import embed_in_surface
    fr = embed_in_surface(scaled_frame(fmt, name, fov_s=1.2, seed=0x6EC0 + interp, interpolation=interp, background_rgba=(0.2, 0.6, 0.4, 1.0)), (40, 14), (20, 6))
    ref = O.run_frame(fr)
    got = warp.run_frame(fr, jit=jit)
    assert warp.last_backend().startswith("yuv_fused") and warp.last_backend().endswith("_jit") == (jit == 2), warp.last_backend()
    compare(ref, got, fr, "%s %s window of a surface" % (name, fmt))
    assert_outside_untouched(fr, got)


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12", "RGBA"])
def test_downscaled_output_with_stride_padding(fmt):
    fr = scaled_frame(fmt, "down_half", seed=0x57D0, stride_align=1024)
    assert all(pl["out_size"][2] > pl["out_size"][0] * pl["params"].bytes_per_pixel for pl in fr.planes)    # every output row has padding behind it
    ref = O.run_frame(fr)
    for jit in (0, 2):
        got = warp.run_frame(fr, jit=jit)
        assert warp.last_backend().startswith("yuv_fused") and warp.last_backend().endswith("_jit") == (jit == 2), warp.last_backend()
        compare(ref, got, fr, "%s stride padding, jit %d" % (fmt, jit))
        assert_outside_untouched(fr, got)


# ---- eligibility edges in the output size -------------------------------------------------------------------------------------------------------------------
def _wide_frame(out_w):
    return S.SyntheticFrame("YUV422P16LE", 640, 8, seed=0x10000 + out_w, fov=640.0 / out_w, out_size=(out_w, 8), readout_ms=16.0)


def test_output_width_65536_is_fused_without_the_certified_pass():
    """65536 = 2^16: the int_products_exact identities hold (odd part 1), so the frame is fused; the first pass parks deferred pixels as x | y << 16, so an
    output wider than 65535 takes the exact first pass."""
    fr = _wide_frame(65536)
    assert fr.matrices.shape[0] == 8
    be0, be2 = check_scaled(fr, True, "65536 x 8")
    assert (be0, be2) == ("yuv_fused", "yuv_fused_jit"), (be0, be2)


def test_output_width_65600_takes_the_per_plane_kernel():
    """65600 = 2^6 x 1025: (65600 - 1) x 1025 >= 2^24, the luma identity x * ow / ow = x is no longer exact in f32 — the per-plane kernel's, bit-exact."""
    check_scaled(_wide_frame(65600), False, "65600 x 8")
