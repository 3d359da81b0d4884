"""gfw_undistort_clip_params on the CPU tier: the per-frame flavour of the fused kernel (GFW_JIT_PERFRAME), its own source interpreted on the host
(tests/_emu_perframe.py), runs ONE launch of frames whose KernelParams move from frame to frame — the adaptive-zoom fov and its centre (translation2d),
keyframed lens correction, background margin and feather, the render loop's fill flag.  Every frame must be the oracle's for that frame's own params."""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S
import _clip_sweep as CS
import _emu as E
import _emu_perframe as EP
import _oracle as O
from test_gpu_lens_models import DIGITAL

W, H = 160, 96


def clip(fmt, n, fov, t2, overrides=None, fill=(), seed=0x7C10, **kw):
    """n frames of one lens: frame f with fov(f), translation2d t2(f), base_overrides overrides(f), FILL_WITH_BACKGROUND on the frames in `fill`"""
    frames = []
    for f in range(n):
        base = dict(overrides(f) if overrides else {})
        base["translation2d"] = t2(f)
        frames.append(S.SyntheticFrame(fmt, W, H, seed=seed + f, timestamp_ms=1000.0 + 33.3 * f, fov=fov(f), base_overrides=base,
                                       flags=abi.FLAG_FILL_WITH_BACKGROUND if f in fill else 0, **kw))
    return frames


def same_as_oracle_per_frame(frames):
    got = EP.run_frames_pf(frames)
    for f, fr in enumerate(frames):
        for p, (a, b) in enumerate(zip(O.run_frame(fr), got[f])):
            assert np.array_equal(a, b), "frame %d plane %d: %d bytes differ" % (f, p, int(np.count_nonzero(np.asarray(a) != np.asarray(b))))
    return got


def moving_centre(f):
    return (-6.5 + 2.75 * f, 4.25 - 1.5 * f)


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12", "RGBA"])
def test_dynamic_zoom_on_the_lean_fisheye_body(fmt):
    """fov and the zoom centre differ on every frame; frames 2 and 4 are filled with the background"""
    frames = clip(fmt, 6, lambda f: 1.0 + 0.06 * f, moving_centre, fill=(2, 4), background_rgba=(0.2, 0.4, 0.6, 1.0))
    got = same_as_oracle_per_frame(frames)
    assert not np.array_equal(got[0][0], got[1][0])


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12", "RGBA"])
def test_keyframed_lens_correction_on_the_generic_body(fmt):
    """lens_correction_amount < 1 on every frame, moving with the fov (the blend's unzoom reads both); frame 3 filled"""
    frames = clip(fmt, 5, lambda f: 1.05 + 0.05 * f, moving_centre, overrides=lambda f: {"lens_correction_amount": 0.3 + 0.15 * f}, fill=(3,))
    same_as_oracle_per_frame(frames)


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12", "RGBA"])
def test_background_margin_and_feather_per_frame(fmt):
    """background mode 3 with a margin and feather of each frame's own"""
    frames = clip(fmt, 5, lambda f: 1.2 + 0.04 * f, moving_centre,
                  overrides=lambda f: {"background_mode": 3, "background_margin": 0.05 + 0.03 * f, "background_margin_feather": 0.12 - 0.02 * f},
                  fill=(0,), background_rgba=(0.9, 0.1, 0.3, 1.0))
    same_as_oracle_per_frame(frames)


def test_the_flavour_reads_each_frames_own_slot():
    """the control: the same launch with every frame given frame 0's slot is NOT the oracle's for the frames that moved (the slots are what the kernel reads)"""
    frames = clip("NV12", 3, lambda f: 1.0 + 0.08 * f, moving_centre)
    got = EP.run_frames_pf(frames)
    saved = EP.slot_of
    try:
        EP.slot_of = lambda fr: saved(frames[0])
        wrong = EP.run_frames_pf(frames)
    finally:
        EP.slot_of = saved
    assert np.array_equal(got[0][0], wrong[0][0])
    assert not np.array_equal(got[2][0], wrong[2][0])


# ---- the audit build of the flavour, random per-frame clips (gfw_undistort_clip_params under GFW_OPT_KERNEL_VARIANT 3 / 4) ------------------------------------
# jit_for sends the audit of a per-frame launch to the flavour's own audit build (GFW_JIT_AUDIT=1): the certificate half-width E of each frame comes from that
# frame's own translation2d, which no ahead-of-time instantiation knows.  The audit build leaves out the fast row (gfw_frame.hip: !AUDIT), so the audit speaks for
# the certificates and the first pass; the parity of every frame with the oracle speaks for the pixels.

SWEEP_FORMATS = ["NV12", "P010LE", "YUV420P", "YUV422P16LE", "YUV444P16LE", "RGBA", "RGBAF32", "RGBAF16"]
SWEEP_MODELS = ["opencv_fisheye", "gopro", "sony", "generic_polynomial"]
SWEEP_SIZES = [(160, 96), (320, 180), (480, 270), (640, 360), (960, 540), (1280, 720)]
SWEEP_SEEDS = 8                                                             # (one of each format; two minutes for the new CPU tests)
FULL_HD_SEEDS = (3, 6)                                                      # the lattice form of the first pass: taken at 1920 x 1080, rejected below


def sweep_clip(seed):
    """one launch of 3-6 frames: a lens model, format, sampler (in turn), shutter direction and readout per seed; fov, zoom centre and fill flag per frame
    (_clip_sweep); the two full-HD seeds are fisheye clips (the lattice form is the fisheye's)"""
    rng = np.random.default_rng(0xC11F + seed)
    w, h = (1920, 1080) if seed in FULL_HD_SEEDS else SWEEP_SIZES[int(rng.integers(0, len(SWEEP_SIZES)))]
    model = "opencv_fisheye" if seed in FULL_HD_SEEDS else SWEEP_MODELS[seed % 4]
    lens = CS.fisheye_lens(rng, w, h) if model == "opencv_fisheye" else dict(CS.lens_for(model, w, h))
    fmt, interp = SWEEP_FORMATS[seed % 8], (2, 4, 8)[seed % 3]
    hrs = bool(rng.integers(0, 2))
    readout = float(rng.uniform(-30.0, 30.0))
    n = 3 if (w, h) == (1920, 1080) else int(rng.integers(3, 7))
    fovs, t2s, fills = CS.motion(rng, n, w, h)
    frames = [S.SyntheticFrame(fmt, w, h, seed=0x5EED + 13 * seed + f, timestamp_ms=1000.0 + 33.3 * f, lens=lens, fov=fovs[f], readout_ms=readout,
                                horizontal_rs=hrs, interpolation=interp, base_overrides={"translation2d": t2s[f]},
                                flags=abi.FLAG_FILL_WITH_BACKGROUND if fills[f] else 0, background_rgba=(0.3, 0.6, 0.1, 1.0)) for f in range(n)]
    return frames, "%s %dx%d %s interp %d %s readout %.1f, %d frames, fill %s" % (model, w, h, fmt, interp, "hrs" if hrs else "vrs", readout, n,
                                                                                  [f for f in range(n) if fills[f]])


def check_audit_words(a, frames, what):
    """no wrong certificate, nothing out of range, no queue overflow; where the launch has a certified pass every pixel of every frame that takes it is counted
    once (a filled frame has no first pass) and the measured gap lies inside E"""
    assert a["wrong"] == 0 and a["out_of_range"] == 0 and a["queue_overflow"] == 0, (what, a)
    if a["fast1"]:
        p0 = frames[0].planes[0]["params"]
        taking = sum(1 for fr in frames if not fr.planes[0]["params"].flags & abi.FLAG_FILL_WITH_BACKGROUND)
        assert a["certified"] + a["queued"] == p0.output_width * p0.output_height * taking, (what, a, taking)
        if taking:
            assert a["eps_px"] > 0.0 and a["gap_px"] < a["eps_px"], (what, a)


@pytest.mark.parametrize("seed", range(SWEEP_SEEDS))
def test_random_per_frame_clip_is_exact_and_its_audit_clean(seed):
    frames, what = sweep_clip(seed)
    audit = EP.library_key(frames, audit=True) is not None                  # (no table derivable for the lens: the ahead-of-time audit, not this flavour's)
    res = EP.run_frames_pf(frames, audit=audit)
    got, a = res if audit else (res, None)
    for f, fr in enumerate(frames):
        for p, (x, y) in enumerate(zip(O.run_frame(fr), got[f])):
            assert np.array_equal(x, y), "%s: frame %d plane %d: %d bytes differ" % (what, f, p, int(np.count_nonzero(np.asarray(x) != np.asarray(y))))
    if a is not None:
        check_audit_words(a, frames, what)
        print("%s: certified %d, queued %d, gap %.3g, E %s" % (what, a["certified"], a["queued"], a["gap_px"], a["eps_px"]))


def test_the_sweep_reaches_the_lattice_form_and_every_family():
    """(what the seeds above cover, pinned: every lens model, format and sampler, both shutter directions, the certified pass on most seeds)"""
    seen = [sweep_clip(s) for s in range(SWEEP_SEEDS)]
    fr0s = [frames[0] for frames, _ in seen]
    assert {fr.lens["model"] for fr in fr0s} == set(SWEEP_MODELS)
    assert {fr.planes[0]["params"].interpolation for fr in fr0s} == {2, 4, 8} and {fr.fmt for fr in fr0s} == set(SWEEP_FORMATS)
    assert {bool(fr.planes[0]["params"].flags & abi.FLAG_HORIZONTAL_RS) for fr in fr0s} == {False, True}
    assert sum(1 for fr in fr0s if fr.width == 1920) == 2
    assert sum(1 for frames, _ in seen if EP._envelope_table(frames)[0] is not None) >= 6


# ---- bodies of the flavour with per-frame fov, zoom centre and amount ---------------------------------------------------------------------------------------


def body_clip(fmt, n, lens_kw=None, overrides=None, fov=lambda f: 1.05 + 0.05 * f, ibis=False, **kw):
    lens = dict(S.gopro_style_lens(W, H), **(lens_kw or {}))
    frames = []
    for f in range(n):
        base = dict(overrides(f) if overrides else {})
        base["translation2d"] = moving_centre(f)
        fr = S.SyntheticFrame(fmt, W, H, seed=0x7B00 + f, timestamp_ms=1000.0 + 33.3 * f, lens=lens, fov=fov(f), base_overrides=base, **kw)
        if ibis:                                             # IBIS / OIS terms in the rows (tests/test_gpu_lens_models.py test_ibis_terms_with_device_resident_matrices)
            y = np.arange(fr.matrices.shape[0], dtype=np.float32)
            fr.matrices[:, 9] = 1.25 * np.sin(y * 0.05 + f)
            fr.matrices[:, 10] = -0.7 * np.cos(y * 0.03)
            fr.matrices[:, 11] = 0.05 * np.sin(y * 0.02) + 0.01
            fr.matrices[:, 12] = 0.5
            fr.matrices[:, 13] = -0.25
            fr.matrices[::7, 9:14] = 0.0
        frames.append(fr)
    return frames


@pytest.mark.parametrize("digital", sorted(DIGITAL))
def test_digital_lenses_under_dynamic_zoom(digital):
    frames = body_clip("NV12", 4, lens_kw={"digital": digital}, overrides=lambda f: {"digital_lens_params": DIGITAL[digital]})
    assert all(E.feature_bits(fr) == 2 for fr in frames)
    same_as_oracle_per_frame(frames)


@pytest.mark.parametrize("fmt", ["NV12", "RGBAF32"])
def test_digital_lens_with_keyframed_lens_correction(fmt):
    """the blend's unzoom reads the frame's own fov and amount (gfw_warp.h) under a digital lens"""
    frames = body_clip(fmt, 4, lens_kw={"digital": "gopro_superview"}, overrides=lambda f: {"lens_correction_amount": 0.3 + 0.15 * f}, fov=lambda f: 1.0 + 0.07 * f)
    assert all(E.feature_bits(fr) == 2 | 8 for fr in frames)
    same_as_oracle_per_frame(frames)


def test_refraction_with_keyframed_amount():
    frames = body_clip("YUV422P16LE", 4, overrides=lambda f: {"light_refraction_coefficient": 1.33, "lens_correction_amount": 0.4 + 0.15 * f}, flags=abi.FLAG_ANY_UNDERWATER)
    assert all(E.feature_bits(fr) == 4 | 8 for fr in frames)
    same_as_oracle_per_frame(frames)


def test_ibis_rows_under_dynamic_zoom():
    frames = body_clip("YUV422P16LE", 4, ibis=True, flags=abi.FLAG_HAS_IBIS_DATA)
    assert all(E.feature_bits(fr) == 1 for fr in frames)
    same_as_oracle_per_frame(frames)


def test_background_mode_3_under_a_horizontal_shutter():
    frames = body_clip("P010LE", 4, overrides=lambda f: {"background_mode": 3, "background_margin": 0.04 + 0.02 * f, "background_margin_feather": 0.1 - 0.02 * f},
                       fov=lambda f: 1.25 + 0.04 * f, horizontal_rs=True, background_rgba=(0.7, 0.2, 0.5, 1.0))
    assert all(E.feature_bits(fr) == 16 for fr in frames)
    same_as_oracle_per_frame(frames)


# ---- E per frame --------------------------------------------------------------------------------------------------------------------------------------------
def shifted(shift, seed, fmt="YUV422P16LE", w=640, h=360):
    """tests/test_emu_pass1_audit.py shifted_frame as a frame of a clip: translation2d = (shift, shift), the matrices' constant terms moved the other way (the same
    geometry through coordinates far from the origin; the certificate's matrix-dependent part grows with |translation2d|)"""
    fr = S.SyntheticFrame(fmt, w, h, seed=seed, timestamp_ms=1000.0 + 33.3 * (seed - 3), base_overrides={"translation2d": (shift, shift)})
    m, t = fr.matrices, np.float32(shift)
    for col in (0, 3, 6):
        m[:, col + 2] -= t * m[:, col] + t * m[:, col + 1]
    return fr


def mixed_shift_frames():
    return [shifted(0.0, 3), shifted(250.0, 4), shifted(-200.0, 5)]


def test_the_launch_certifies_each_frame_with_its_own_translation():
    """Audit word 6 is the largest E the launch's frames used.  Each frame's own E comes from a one-frame launch given the MIXED launch's table (so that only the
    frame's own translation2d and matrix differ): the mixed launch's word must be the largest of them, and that must not be frame 0's — a kernel that certified
    every frame with frame 0's translation2d would report frame 0's E for the launch."""
    frames = mixed_shift_frames()
    table, _ = EP._envelope_table(frames)
    assert table is not None
    got, a = EP.run_frames_pf(frames, audit=True)
    check_audit_words(a, frames, "mixed shifts")
    own = []
    for f, fr in enumerate(frames):
        assert all(np.array_equal(x, y) for x, y in zip(O.run_frame(fr), got[f])), f
        _, af = EP.run_frames_pf([fr], audit=True, table=table)
        check_audit_words(af, [fr], "frame %d alone" % f)
        own.append(af["eps_word"])
    print("E per frame", [float(np.array([w], np.uint32).view(np.float32)[0]) for w in own], "launch", a["eps_px"])
    assert a["eps_word"] == max(own), (a["eps_word"], own)
    assert int(np.argmax(own)) != 0 and own[int(np.argmax(own))] > own[0], own


def test_the_host_certifies_at_least_40_of_the_device_sweeps_clips():
    """The device audit sweep (tests/test_gpu_clip_params_cover.py, tests/_clip_sweep.py gpu_clips) needs at least 40 of its 60 clips served by the certified first
    pass; whether the host certifies a clip is decided here, by the library's own key of the call's first launch on device-resident tables (the envelope of the
    call's fov and zoom centre).  49 of 60 are certified today (declined: 5 fisheye clips, 6 GoPro ones — wide fields of view); a change in that decision fails
    here before any GPU minute."""
    served = sum(1 for _, frames in CS.gpu_clips() if EP.library_key(frames, matrices_on_device=2)[0]["GFW_JIT_FAST1"] == "1")
    assert served >= 40, served


# ---- the lattice form's fallback ---------------------------------------------------------------------------------------------------------------------------
def device_rho(frames):
    """the first pass's table range on device-resident tables (gfw_api_certificate.inc p1_setup, a fresh context): the corner ray of the call's envelope of fov
    and zoom centre plus 15 degrees, with the table's head-room"""
    import math
    ps = [fr.planes[0]["params"] for fr in frames]
    hx = max(0.5 * p.output_width * p.fov / abs(p.f[0]) + abs(p.translation2d[0]) * p.fov / abs(p.f[0]) for p in ps)
    hy = max(0.5 * p.output_height * p.fov / abs(p.f[1]) + abs(p.translation2d[1]) * p.fov / abs(p.f[1]) for p in ps)
    ang = math.atan(math.hypot(hx, hy)) + 0.26
    return min((math.tan(ang) ** 2 if ang < 1.45 else 64.0) * 1.15, 64.0)


def test_a_rejected_lattice_keeps_the_per_pixel_half_width():
    """Regression (clip 58 of the device audit sweep, frame 0: a 960x540 fisheye turned by up to 15 degrees on a device-resident table).  The lattice form's
    nodes reach a tile beyond the frame (+128, +32 px here), and E over that extent is 0.2024 px; the frame's own pixels give 0.1960.  The lattice was rejected
    (E above GFW_P1_LATTICE_MAX_E) and the frame fell back to the per-pixel form — with the nodes' E, 0.2 px or more, so not one pixel was certified where the
    per-pixel form (GFW_OPT_KERNEL_VARIANT 4) certifies two thirds of them.  A rejected lattice must leave exactly the per-pixel form's result."""
    _, frames = next(c for i, c in enumerate(CS.gpu_clips()) if i == 58)
    fr = frames[0]
    for pl, q in zip(fr.planes, S.SyntheticFrame(fr.fmt, fr.width, fr.height, seed=5).planes):       # (the sweep's frames are geometry only)
        pl["src"], pl["dst"] = q["src"], q["dst"]
    p0 = fr.planes[0]["params"]
    table = E.p1_table(p0, fr.matrices, p0.matrix_count, rho_max=device_rho(frames))
    assert table is not None
    res = {}
    for per_pixel in (0.0, 1.0):
        t = table[:4] + (table[4].copy(),)
        t[4][5] = per_pixel
        got, a = EP.run_frames_pf([fr], audit=True, table=t)
        check_audit_words(a, [fr], "p1_lat[5] = %g" % per_pixel)
        assert all(np.array_equal(x, y) for x, y in zip(O.run_frame(fr), got[0])), per_pixel
        res[per_pixel] = (a["certified"], a["queued"], a["eps_word"])
    print("lattice-eligible", res[0.0], "per-pixel form", res[1.0])
    assert res[1.0][0] > 0.5 * fr.width * fr.height, res
    assert res[0.0] == res[1.0], res
