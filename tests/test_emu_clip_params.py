"""gfw_undistort_clip_params on the CPU tier: the per-frame flavour of the fused kernel (GFW_JIT_PERFRAME), its own source interpreted on the host
(tests/_emu_perframe.py), runs ONE launch of frames whose KernelParams move from frame to frame — the adaptive-zoom fov and its centre (translation2d),
keyframed lens correction, background margin and feather, the render loop's fill flag.  Every frame must be the oracle's for that frame's own params."""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S
import _emu_perframe as EP
import _oracle as O

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
