"""gfw_undistort_clip_params on the MI355X beyond one 320x192 launch: the audit of the per-frame flavour's certified first pass over 60 random clips up to 8K,
E taken per frame, full-size clips over several launches (the lattice form included), the flavour's bodies x formats x samplers, launches split by the cap,
frames that cannot join a launch, ordering and overlap, a mid-call error and checksum rings across launches.

Every output is compared with the oracle fed that frame's own params and source, bit for bit (assert_plane_equal, as the rest of the GPU tier).  Every case
asserts its backend and its launch count EXACTLY, derived from the contract: gfw_debug_frames_per_launch for the cap, gfw_debug_jit_key_clip_params (the library's
own key for the call's first launch, without a device) for whether the host certifies the first pass.

The audit build leaves out the fast row of the kernel (gfw_frame.hip: !AUDIT): the audits speak for the certificates and the first pass; the parity cases speak
for the pixels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _clip_sweep as CS
import _emu_perframe as EP
import _oracle as O
from test_gpu_parity import assert_plane_equal
from test_gpu_fullsize import _View
from test_gpu_lens_models import DIGITAL
from test_gpu_scaled_output import check_audit

pytestmark = pytest.mark.gpu

W, H = 320, 192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_OUTPUT_BUFFER_EMPTY = -6                                                # (include/gfwarp.h GFW_ERR_OUTPUT_BUFFER_EMPTY)


def bytes_per_frame(fr):
    """source + destination bytes of a frame as clip_launch_limit counts them (stride x rows of every plane, both sides)"""
    return sum(pl["size"][2] * pl["size"][1] + pl["out_size"][2] * pl["out_size"][1] for pl in fr.planes)


def per_launch(frames, budget=0):
    return abi.load_library().gfw_debug_frames_per_launch(bytes_per_frame(frames[0]), budget, len(frames))


def shares(frames, budget=0):
    """launches of a call whose frames all join: ceil(n / frames per launch)"""
    k = per_launch(frames, budget)
    return -(-len(frames) // k)


def certified(frames):
    """whether the library certifies the first pass of the call's first launch on device-resident tables (its own key, no device)"""
    key = EP.library_key(frames, matrices_on_device=2)
    return key is not None and key[0]["GFW_JIT_FAST1"] == "1"


def expect_backend(frames):
    return "yuv_fused_p1_jit" if certified(frames) else "yuv_fused_jit"


def clip(n, fov=lambda f: 1.0 + 0.02 * f, t2=lambda f: (-9.5 + 1.75 * f, 6.25 - 1.25 * f), overrides=None, fill=(), fmt="YUV422P16LE", lens=None, w=W, h=H,
         interp=lambda f: 2, flags=0, seed=0x5E60, **kw):
    """n frames of one lens: frame f with fov(f), zoom centre t2(f), base_overrides overrides(f), sampler interp(f), FILL_WITH_BACKGROUND on the frames in `fill`"""
    frames = []
    for f in range(n):
        base = dict(overrides(f) if overrides else {})
        base["translation2d"] = t2(f)
        frames.append(S.SyntheticFrame(fmt, w, h, seed=seed + f, timestamp_ms=1000.0 + 33.3 * f, fov=fov(f), base_overrides=base, pixels=False, lens=lens,
                                       interpolation=interp(f), flags=flags | (abi.FLAG_FILL_WITH_BACKGROUND if f in fill else 0), **kw))
    return frames


def run(frames, variant=0, jit=2, mod=2, host=(), zeros=False, ring=0, chain=False, write_back=False, empty=None, use_clip=True):
    """frames on one context through gfw_undistort_clip_params (use_clip) or gfw_undistort_frame frame by frame.  Device buffers and packed device tables
    (mod 2) unless: `host` frames use HOST buffers, mod = 0 host rows[14] tables.  chain: frame f + 1 reads frame f's destination; write_back: frame f + 1
    writes frame f's source; empty: that frame's output is declared empty (a validation error); ring: a checksum ring of that many words.
    -> dict(rc, backend, status, launches, covered, audit, outs, srcs, sums)"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(frames)
    if zeros:
        d_src = [[torch.zeros(pl["size"][2] * pl["size"][1], dtype=torch.uint8, device=dev) for pl in fr.planes] for fr in frames]
    else:
        d_src = [fr.device_planes(dev) for fr in frames]
    d_dst = [fr.device_outputs(dev) for fr in frames]
    if chain:
        d_src = [d_src[0]] + d_dst[:-1]
    if write_back:
        d_dst = [d_dst[0]] + d_src[:-1]
    torch.cuda.synchronize(dev)
    srcs = [[t.cpu().numpy().copy() for t in d] for d in d_src]            # (what each frame reads — before anything is written)
    h_src = {j: [s.copy() for s in srcs[j]] for j in host}
    h_dst = {j: [np.full(pl["out_size"][2] * pl["out_size"][1], 0x5A, dtype=np.uint8) for pl in frames[j].planes] for j in host}
    d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
    d_sums = torch.zeros(max(ring, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [[pl["params"] for pl in fr.planes] for fr in frames]
    bufs = []
    for j, fr in enumerate(frames):
        fb = []
        for p, pl in enumerate(fr.planes):
            if j in host:
                fb.append(warp.host_buffers(h_src[j][p], pl["size"], h_dst[j][p], pl["out_size"]))
            else:
                fb.append(warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], d_dst[j][p].data_ptr(),
                                              0 if (j == empty and p == 0) else d_dst[j][p].numel(), pl["out_size"]))
        bufs.append(fb)
    rows = frames[0].matrices.shape[0]
    mats = [m.data_ptr() for m in d_mat] if mod else [fr.matrices for fr in frames]
    be = warp.Backend(params[0][0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    rc = 0
    try:
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, mod)
        be.set_option(abi.OPT_JIT, jit)
        be.set_option(abi.OPT_PROFILE, 1)
        if variant:
            be.set_option(abi.OPT_KERNEL_VARIANT, variant)
            be.get_audit(reset=True)
        if ring:
            be.set_frame_checksums(d_sums.data_ptr(), ring)
        if use_clip:
            call = warp.ClipParamsCall(be, bufs, params, types, mats, rows)
            rc = call.fn(be.ctx, call.nf, call.n, call.barr, call.parr, call.tarr, call.marr, call.mc)
        else:
            for j in range(n):
                fc = warp.FrameCall(be, bufs[j], params[j], types, mats[j], rows)
                rc = fc.fn(be.ctx, fc.n, fc.barr, fc.parr, fc.tarr, fc.mp, fc.mc, None, 0)
                if rc:
                    break
        be.synchronize()
        backend, status = warp.Backend.last_backend_of(be), be.jit_status()
        _, launches, covered = be.get_profile_frames()
        audit = be.get_audit_full() if variant else None
        if ring:
            be.set_frame_checksums(0, 0)
    finally:
        be.close()
    torch.cuda.synchronize(dev)
    outs = []
    for j in range(n):
        outs.append(h_dst[j] if j in host else [t.cpu().numpy() for t in d_dst[j]])
    return dict(rc=rc, backend=backend, status=status, launches=launches, covered=covered, audit=audit, outs=outs, srcs=srcs,
                sums=[int(v) & 0xFFFFFFFFFFFFFFFF for v in d_sums.cpu().numpy().tolist()][:ring])


def exact(frames, got, what, refs=None, only=None):
    for j, fr in enumerate(frames):
        if only is not None and j not in only:
            continue
        ref = refs[j] if refs is not None else O.run_frame(_View(fr, got["srcs"][j]))
        for p, (a, b) in enumerate(zip(ref, got["outs"][j])):
            assert_plane_equal(a, b, fr.planes[p]["pixel_type"], "%s, frame %d plane %d" % (what, j, p))


# ---- D.1: the audit of the flavour over 60 random clips -------------------------------------------------------------------------------------------------------
def taking(frames):
    """frames of the call that take the first pass (a filled frame takes none)"""
    return sum(1 for fr in frames if not fr.planes[0]["params"].flags & abi.FLAG_FILL_WITH_BACKGROUND)


def test_sixty_random_per_frame_clips_never_produce_a_wrong_certificate():
    """tests/_clip_sweep.py gpu_clips: per-frame fov and zoom centre, fill flags, rotations and readouts, fisheye / GoPro / Sony / generic polynomial, 320x180 to
    8K, 4-16 frames, through gfw_undistort_clip_params on device-resident tables under GFW_OPT_KERNEL_VARIANT 3 (every third clip also 4).  Pixel content is
    irrelevant here (zero planes).  A served clip (the host certifies its first pass: the library's own key says which, and the run must agree) takes the
    flavour's audit build in shared launches; its audit must be clean and count every pixel of every frame that takes the first pass once."""
    served, worst, declined = 0, 0.0, []
    for i, (model, frames) in enumerate(CS.gpu_clips()):
        fr0 = frames[0]
        w, h, n = fr0.width, fr0.height, len(frames)
        want = certified(frames)
        for variant in ((3, 4) if i % 3 == 0 else (3,)):
            what = "clip %d: %s %dx%d %s, %d frames, variant %d" % (i, model, w, h, fr0.fmt, n, variant)
            got = run(frames, variant=variant, jit=1, zeros=True)
            a = got["audit"]
            assert got["rc"] == 0, (what, got["rc"])
            assert a["certified1_wrong"] == 0 and a["out_of_range"] == 0, (what, a)
            if not want:
                assert got["backend"] in ("yuv_fused_jit", "yuv_fused"), (what, got["backend"])
                declined.append((i, model, w, h))
                break
            assert got["backend"] == "yuv_fused_p1_jit", (what, got["backend"])
            assert got["launches"] == shares(frames) and got["covered"] == n, (what, got["launches"], got["covered"], per_launch(frames))
            check_audit(a, w * h * taking(frames), what)
            worst = max(worst, a["pass1_gap_px"] / a["pass1_eps_px"])
        served += 1 if want else 0
    print("per-frame audit sweep: %d of 60 clips served, declined %s; worst gap / E = %.3f" % (served, declined, worst))
    assert served >= 40, (served, declined)


# ---- D.2: E per frame on the device ------------------------------------------------------------------------------------------------------------------------
def shifted(shift, seed, w=640, h=360):
    """tests/test_emu_clip_params.py shifted: translation2d (shift, shift), the matrices compensated (the same geometry far from the origin)"""
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=seed, timestamp_ms=1000.0 + 33.3 * (seed - 3), base_overrides={"translation2d": (shift, shift)}, pixels=False)
    m, t = fr.matrices, np.float32(shift)
    for col in (0, 3, 6):
        m[:, col + 2] -= t * m[:, col] + t * m[:, col + 1]
    return fr


def test_the_certificate_follows_each_frames_own_translation_on_the_device():
    """The CPU tier's mixed-shift launch (t2 = 0, 250, -200 px at 640x360: the 250 px frame has the largest E there) through clip_params on device tables,
    variant 4, in two orders: unshifted frame first and 250 px frame first.  Same frames, same envelope: word 6 (the largest E) must be the same in both and the
    outputs bit-exact.  A kernel that certified every frame with frame 0's translation would report a different E for the two orders: on this call's table the
    frames' own E are 0.1222 (unshifted), 0.1271 (250 px) and 0.1195 (-200 px) by the host-side restatement, and the device reports 0.1271 in both orders."""
    a, b, c = shifted(0.0, 3), shifted(250.0, 4), shifted(-200.0, 5)
    words = []
    for order in ([a, b, c], [b, a, c]):
        assert certified(order)
        got = run(order, variant=4)
        what = "order %s" % [fr.planes[0]["params"].translation2d[0] for fr in order]
        assert got["backend"] == "yuv_fused_p1_jit" and got["launches"] == 1 and got["covered"] == 3, (what, got["backend"], got["launches"])
        check_audit(got["audit"], 640 * 360 * 3, what)
        exact(order, got, what)
        words.append(got["audit"]["pass1_eps_px"])
    print("largest E: unshifted first %.6f, 250 px first %.6f" % tuple(words))
    assert words[0] == words[1], words


# ---- D.3: full size ----------------------------------------------------------------------------------------------------------------------------------------
def full_clip(n, w, h, seed):
    """bench.py's C2 shape (4:2:2 16-bit, the GoPro-style fisheye, 16 ms readout) with the adaptive zoom moving fov and centre every frame.  (The fov stays below
    0.9: on device-resident tables the table's range follows the envelope's corner ray plus 15 degrees, and beyond fov 1.1 or so the per-pixel E of a 4K frame
    passes GFW_P1_LATTICE_MAX_E — the lattice form could not be taken at all.)"""
    return [S.SyntheticFrame("YUV422P16LE", w, h, seed=seed + f, timestamp_ms=1000.0 + 33.3 * f, fov=0.8 + 0.005 * f,
                             base_overrides={"translation2d": (-24.0 + 3.0 * f, 13.5 - 1.5 * f)}, pixels=False) for f in range(n)]


@pytest.mark.parametrize("n,w,h", [(18, 3840, 2160), (6, 7680, 4320)])
def test_full_size_dynamic_zoom_leaves_in_capped_launches(n, w, h):
    """18 4K frames: two launches of 9 under the 1.1 GB cap; 6 8K frames: two launches of 3.  Every frame equals the oracle and the frame-by-frame run."""
    frames = full_clip(n, w, h, 0x4C00 + w)
    k = per_launch(frames)
    assert (k, shares(frames)) == ({3840: 9, 7680: 3}[w], 2)
    got = run(frames)
    assert got["backend"] == expect_backend(frames) == "yuv_fused_p1_jit" and got["launches"] == 2 and got["covered"] == n, (got["backend"], got["launches"])
    fbf = run(frames, jit=0, use_clip=False)
    refs = [O.run_frame(_View(fr, got["srcs"][j])) for j, fr in enumerate(frames)]
    exact(frames, got, "%dx%d clip_params" % (w, h), refs=refs)
    exact(frames, fbf, "%dx%d frame by frame" % (w, h), refs=refs)


def test_the_4k_clip_takes_the_lattice_form():
    """The same 4K clip under variant 3 (the lattice form where the curvature term admits it) reports a LARGER word 6 than under variant 4 (the per-pixel form):
    the lattice adds its curvature term to the per-pixel E, and a rejected lattice falls back to exactly the per-pixel E (since this change: it used to fall back
    to an E taken over the lattice's extent, which also made this comparison pass where no lattice was taken).  Both audits clean."""
    frames = full_clip(18, 3840, 2160, 0x4C00 + 3840)
    e = {}
    for variant in (3, 4):
        got = run(frames, variant=variant, zeros=True)
        assert got["backend"] == "yuv_fused_p1_jit" and got["launches"] == 2, (variant, got["backend"], got["launches"])
        check_audit(got["audit"], 3840 * 2160 * 18, "4K variant %d" % variant)
        e[variant] = got["audit"]["pass1_eps_px"]
    print("4K largest E: lattice %.5f, per pixel %.5f" % (e[3], e[4]))
    assert e[3] > e[4], e


# ---- D.4: bodies x formats x samplers, one shared launch each ---------------------------------------------------------------------------------------------
FORMATS = ["NV12", "P010LE", "YUV420P", "YUV422P16LE", "YUV444P16LE", "RGBA", "RGBAF32", "RGBAF16"]


def _body_cases():
    """(name, format, sampler, body): every format and sampler with the lean fisheye, then the other bodies with formats and samplers in turn"""
    cases = [("fisheye", fmt, (2, 4, 8)[i % 3], "fisheye") for i, fmt in enumerate(FORMATS)]
    cases += [("fisheye", fmt, (2, 4, 8)[(i + 1) % 3], "fisheye") for i, fmt in enumerate(FORMATS)]
    bodies = ["digital:" + d for d in sorted(DIGITAL)] + ["blend", "blend", "blend", "bg3", "bg3", "bg3", "gopro", "sony", "generic_polynomial",
                                                         "gopro", "sony", "generic_polynomial", "hrs", "hrs", "hrs", "hrs:gopro", "hrs:bg3", "blend:digital"]
    for i, body in enumerate(bodies):
        cases.append((body, FORMATS[(3 * i + 1) % len(FORMATS)], (2, 4, 8)[i % 3], body))
    return cases


def body_frames(body, fmt, interp):
    kw, overrides, lens = {}, None, None
    fill = (3, 8)
    if body.startswith("digital") or body == "blend:digital":
        name = body.split(":")[1] if body.startswith("digital:") else "gopro_superview"
        lens = dict(S.gopro_style_lens(W, H), digital=name)
        amount = (lambda f: 0.35 + 0.05 * f) if body == "blend:digital" else (lambda f: 1.0)
        overrides = lambda f: {"digital_lens_params": DIGITAL[name], "lens_correction_amount": amount(f)}
    elif body == "blend":
        overrides = lambda f: {"lens_correction_amount": 0.3 + 0.05 * f}
    elif body in ("bg3", "hrs:bg3"):
        overrides = lambda f: {"background_mode": 3, "background_margin": 0.04 + 0.005 * f, "background_margin_feather": 0.12 - 0.005 * f}
        kw["background_rgba"] = (0.8, 0.2, 0.4, 1.0)
    elif body in ("gopro", "sony", "generic_polynomial", "hrs:gopro"):
        lens = CS.lens_for(body.split(":")[-1], W, H)
    if body.startswith("hrs"):
        kw["horizontal_rs"] = True
    return clip(12, fov=lambda f: 1.05 + 0.02 * f, overrides=overrides, fill=fill, fmt=fmt, lens=lens, interp=lambda f: interp,
                background_rgba=kw.pop("background_rgba", (0.1, 0.5, 0.9, 1.0)), **kw)


@pytest.mark.parametrize("name,fmt,interp,body", _body_cases())
def test_bodies_formats_and_samplers_share_one_launch(name, fmt, interp, body):
    frames = body_frames(body, fmt, interp)
    assert shares(frames) == 1
    got = run(frames)
    what = "%s %s interp %d" % (body, fmt, interp)
    assert got["rc"] == 0 and got["backend"] == expect_backend(frames) and got["launches"] == 1 and got["covered"] == 12, (what, got["backend"], got["launches"])
    exact(frames, got, what)


# ---- D.5: launch splits -------------------------------------------------------------------------------------------------------------------------------------
def test_forty_frames_leave_in_three_launches_every_slot_exact():
    """40 frames at 320x192: 16 per launch at most, dealt evenly — 14 + 13 + 13; frames 14-39 read the slots of launches 2 and 3"""
    frames = clip(40, fov=lambda f: 0.9 + 0.01 * f, t2=lambda f: (-12.0 + 0.6 * f, 7.0 - 0.35 * f), fill=(5, 17, 31))
    assert shares(frames) == 3
    got = run(frames)
    assert got["backend"] == expect_backend(frames) and got["launches"] == 3 and got["covered"] == 40, (got["backend"], got["launches"])
    exact(frames, got, "40 frames")


_CAP_SCRIPT = r"""
import sys, json
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import _oracle as O
import test_gpu_clip_params_cover as T
frames = T.clip(%(n)d, fov=lambda f: 0.95 + 0.01 * f, fill=(2,))
got = T.run(frames)
bad = 0
for j, fr in enumerate(frames):
    for a, b in zip(O.run_frame(T._View(fr, got["srcs"][j])), got["outs"][j]):
        bad += int(np.count_nonzero(np.asarray(a) != np.asarray(b)))
print("RESULT " + json.dumps({"backend": got["backend"], "launches": int(got["launches"]), "covered": int(got["covered"]), "bad": bad}))
"""


def test_a_launch_cap_deals_the_call_over_five_launches(tmp_path):
    """GFW_CLIP_LAUNCH_MB (read once per process: a child interpreter) so small that the 20-frame call needs five launches; the count is the contract's"""
    n = 20
    frames = clip(n, fov=lambda f: 0.95 + 0.01 * f, fill=(2,))
    mb = next(m for m in range(1, 64) if shares(frames, m << 20) == 5)
    script = tmp_path / "cap.py"
    script.write_text(_CAP_SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "n": n})
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GFW_CLIP_LAUNCH_MB=str(mb)), capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and line, (r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(line[-1][7:])
    assert res == {"backend": expect_backend(frames), "launches": 5, "covered": n, "bad": 0}, (res, mb, per_launch(frames, mb << 20))


# ---- D.6: frames that cannot join ---------------------------------------------------------------------------------------------------------------------------
def test_host_buffer_frames_take_single_frame_launches_of_the_call():
    """frames 4 and 9 of 12 on HOST buffers cannot join a launch: they go out alone, on the call's per-frame kernel with their own slot — five launches
    (0-3, 4, 5-8, 9, 10-11)"""
    frames = clip(12, fill=(6,))
    got = run(frames, host=(4, 9))
    assert got["backend"] == expect_backend(frames) and got["launches"] == 5 and got["covered"] == 12, (got["backend"], got["launches"], got["covered"])
    exact(frames, got, "HOST frames 4 and 9")


def test_host_matrix_tables_take_one_launch_per_frame():
    """GFW_OPT_MATRICES_ON_DEVICE 0: the rows[14] tables live on the host — no frame joins a launch"""
    frames = clip(12)
    got = run(frames, mod=0)
    last = EP.library_key(frames[-1:])[0]["GFW_JIT_FAST1"] == "1"          # (host tables: the frame's own first pass, decided on its own rows)
    assert got["backend"] == ("yuv_fused_p1_jit" if last else "yuv_fused_jit") and got["launches"] == 12 and got["covered"] == 12, (got["backend"], got["launches"])
    exact(frames, got, "host tables")


def test_an_ewa_frame_mid_call_runs_per_plane_with_its_own_params():
    """frame 6 of 12 asks for EWA (interpolation 10): the per-plane kernel with that frame's own params (one profiled launch for the frame), the fused frames
    around it in two per-frame launches"""
    frames = clip(12, interp=lambda f: 10 if f == 6 else 2)
    got = run(frames)
    assert got["launches"] == 3 and got["covered"] == 12 and got["backend"] == expect_backend(frames), (got["backend"], got["launches"], got["covered"])
    exact(frames, got, "EWA frame 6")


@pytest.mark.parametrize("what,kw", [
    ("amount reaches 1.0", dict(overrides=lambda f: {"lens_correction_amount": min(1.0, 0.4 + 0.1 * f)})),
    ("sampler changes", dict(interp=lambda f: 2 if f < 6 else 4)),
])
def test_a_new_kernel_mid_call_opens_a_new_launch(what, kw):
    """frames 0-5 and 6-11 differ in a clip constant of the kernel (the blend's feature bit, the sampler): a new launch at frame 6"""
    frames = clip(12, **kw)
    key = [(fr.planes[0]["params"].lens_correction_amount < 1.0, fr.planes[0]["params"].interpolation) for fr in frames]
    assert len(set(key[:6])) == 1 and len(set(key[6:])) == 1 and key[5] != key[6], key
    got = run(frames)
    assert got["launches"] == 2 and got["covered"] == 12 and got["backend"] == expect_backend(frames[6:]), (what, got["backend"], got["launches"])
    exact(frames, got, what)


# ---- D.7: ordering and overlap -----------------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_reads_the_previous_frames_output():
    """frame f + 1's source is frame f's destination: it must see that frame's finished output (one launch per frame), against the oracle chained on its own
    outputs"""
    frames = clip(6, fmt="NV12")
    got = run(frames, chain=True)
    assert got["launches"] == 6 and got["covered"] == 6, got["launches"]
    refs, src = [], got["srcs"][0]
    for fr in frames:
        refs.append(O.run_frame(_View(fr, src)))
        src = refs[-1]
    exact(frames, got, "chained", refs=refs)


def test_a_frame_that_writes_the_previous_frames_source():
    """frame f + 1's destination is frame f's source: frame f must have read it first (one launch per frame)"""
    frames = clip(6, fmt="YUV422P16LE")
    got = run(frames, write_back=True)
    assert got["launches"] == 6 and got["covered"] == 6, got["launches"]
    refs = []
    for j, fr in enumerate(frames):
        v = _View(fr, got["srcs"][j])
        if j > 0:                                    # (the bytes the warp never writes — stride padding — are what that buffer held: frame j - 1's source)
            for p, pl in enumerate(v.planes):
                pl["dst"] = got["srcs"][j - 1][p].copy()
        refs.append(O.run_frame(v))
    exact(frames, got, "write-back", refs=refs)


# ---- D.8: errors and checksums -----------------------------------------------------------------------------------------------------------------------------
def test_a_mid_call_validation_error_keeps_the_frames_before_it():
    """frame 5 of 12 declares an empty output: the call returns the validation error gfw_undistort_frame returns for that frame; frames 0-4 are complete and
    exact (the launch they were in went out before the error), frame 5 and every later frame keep their sentinel bytes"""
    frames = clip(12)
    got = run(frames, empty=5)
    alone = run(frames[5:6], empty=0, use_clip=False)
    assert got["rc"] == alone["rc"] == ERR_OUTPUT_BUFFER_EMPTY, (got["rc"], alone["rc"])
    exact(frames, got, "before the error", only=range(5))
    for j in range(5, 12):
        for p, o in enumerate(got["outs"][j]):
            assert np.all(o == 0x5A), "frame %d plane %d was written" % (j, p)


def test_checksum_ring_across_launches_equals_the_frame_by_frame_run():
    """40 frames (three launches) into a ring of 16 words: each word sums the frames k, k + 16, k + 32 — the same words as the frame-by-frame run"""
    frames = clip(40, fov=lambda f: 0.95 + 0.005 * f, fill=(9, 30))
    got = run(frames, ring=16)
    fbf = run(frames, ring=16, jit=0, use_clip=False)
    assert got["launches"] == 3 and got["backend"] == expect_backend(frames), (got["launches"], got["backend"])
    assert got["sums"] == fbf["sums"] and all(s != 0 for s in got["sums"]), (got["sums"], fbf["sums"])
    exact(frames, got, "checksummed clip")
