"""gfw_undistort_clip_lens on the CPU tier: the moving-lens flavour of the fused kernel (GFW_JIT_PERFRAME=2), its own source interpreted on the host
(tests/_emu_perlens.py), runs ONE launch of frames whose LENS moves from frame to frame — f, c, k and r_limit as a zoom lens or per-frame lens telemetry move
them, a keyframed refraction coefficient, a mesh per frame — beside the fields gfw_undistort_clip_params lets move.  Every frame must be the oracle's for that
frame's own params and mesh."""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S
import _emu as E
import _emu_perlens as EL
import _oracle as O
from _shapes import lens_for
from test_gpu_lens_models import DIGITAL, PHYSICAL, synthetic_mesh

W, H = 160, 96


def moving_centre(f):
    return (-6.5 + 2.75 * f, 4.25 - 1.5 * f)


def zoom_lens(f, n, w=W, h=H, **more):
    """frame f of n of a zoom-lens clip: the focal length runs from 0.47 w to 0.62 w, the principal point wanders by a few pixels, all four k move"""
    t = f / max(n - 1, 1)
    lens = S.gopro_style_lens(w, h)
    fl = (0.47 + 0.15 * t) * w
    lens["f"] = (fl, fl * (1.0 + 0.004 * t))
    lens["c"] = (w / 2.0 + 1.5 * f - 2.0, h / 2.0 - 0.75 * f + 1.0)
    lens["k"] = [0.045 + 0.012 * f, 0.02 - 0.006 * f, -0.02 + 0.004 * f, 0.006 - 0.0015 * f] + [0.0] * 8
    lens.update(more)
    return lens


def clip(fmt, n, lens, fov=lambda f: 1.1, t2=lambda f: (0.0, 0.0), overrides=None, fill=(), flags=0, seed=0x1E50, w=W, h=H, **kw):
    frames = []
    for f in range(n):
        base = dict(overrides(f) if overrides else {})
        base["translation2d"] = t2(f)
        frames.append(S.SyntheticFrame(fmt, w, h, seed=seed + f, timestamp_ms=1000.0 + 33.3 * f, lens=lens(f), fov=fov(f), base_overrides=base,
                                       flags=flags | (abi.FLAG_FILL_WITH_BACKGROUND if f in fill else 0), **kw))
    return frames


_ORACLE = {}


def oracle(fr, mesh=None):
    """the oracle's planes for the frame's own params and mesh (computed once per frame object, shared by the tests and their controls, never written)"""
    key = (id(fr), None if mesh is None else mesh.tobytes())
    if key not in _ORACLE:
        if mesh is None:
            ref = O.run_frame(fr)
        else:
            ref = []
            for pl in fr.planes:
                dst = pl["dst"].copy()
                assert O.undistort_image(pl["src"], pl["size"], dst, pl["out_size"], pl["params"], pl["pixel_type"], fr.model, fr.digital, fr.matrices, mesh=mesh) == 1
                ref.append(dst)
        _ORACLE[key] = (fr, ref)
    return _ORACLE[key][1]


def same_as_oracle_per_frame(frames, meshes=None, what=""):
    got = EL.run_frames_pl(frames, meshes)
    for f, fr in enumerate(frames):
        for p, (a, b) in enumerate(zip(oracle(fr, None if meshes is None else meshes[f]), got[f])):
            assert np.array_equal(a, b), "%s frame %d plane %d: %d bytes differ" % (what, f, p, int(np.count_nonzero(np.asarray(a) != np.asarray(b))))
    return got


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12", "RGBA"])
def test_a_zoom_lens_on_the_lean_fisheye_body(fmt):
    """f, c and all four k differ on every frame, and so do fov and the zoom centre; frame 3 is filled with the background"""
    n = 6
    frames = clip(fmt, n, lambda f: zoom_lens(f, n), fov=lambda f: 1.0 + 0.05 * f, t2=moving_centre, fill=(3,), background_rgba=(0.2, 0.4, 0.6, 1.0))
    assert all(E.feature_bits(fr) == 0 for fr in frames)
    got = same_as_oracle_per_frame(frames, what=fmt)
    assert not np.array_equal(got[0][0], got[1][0])


GENERIC = ["gopro", "sony", "generic_polynomial", "opencv_standard", "poly5"]


def generic_lens(model, f):
    lens = dict(lens_for(model, W, H)) if model in ("gopro", "sony", "generic_polynomial") else S.gopro_style_lens(W, H)
    lens["model"] = model
    k = PHYSICAL[model] + [0.0] * (12 - len(PHYSICAL[model]))
    # each model's own coefficients move: every non-zero one by a few per cent per frame, alternating in sign (the sony / polynomial leading 1.0 and gopro's stay)
    lens["k"] = [v if v in (0.0, 1.0) else v * (1.0 + 0.04 * f * (1 if i % 2 else -1)) for i, v in enumerate(k)]
    lens["f"] = tuple(v * (1.0 + 0.03 * f) for v in lens["f"])
    lens["c"] = (lens["c"][0] + 0.5 * f, lens["c"][1] - 0.25 * f)
    if model == "gopro":
        lens["r_limit"] = 2.5
    return lens


@pytest.mark.parametrize("model", GENERIC)
def test_the_generic_body_under_a_moving_lens(model):
    frames = clip("NV12", 5, lambda f: generic_lens(model, f), fov=lambda f: 1.15 + 0.03 * f, t2=moving_centre)
    assert len({tuple(fr.planes[0]["params"].k) for fr in frames}) == 5
    same_as_oracle_per_frame(frames, what=model)


def test_a_digital_lens_under_a_moving_physical_lens():
    n = 5
    frames = clip("NV12", n, lambda f: zoom_lens(f, n, digital="gopro_superview"), fov=lambda f: 1.05 + 0.04 * f, t2=moving_centre,
                  overrides=lambda f: {"digital_lens_params": DIGITAL["gopro_superview"]})
    assert all(E.feature_bits(fr) == 2 for fr in frames)
    same_as_oracle_per_frame(frames)


def test_a_keyframed_refraction_coefficient():
    n = 5
    frames = clip("YUV422P16LE", n, lambda f: S.gopro_style_lens(W, H), t2=moving_centre, flags=abi.FLAG_ANY_UNDERWATER,
                  overrides=lambda f: {"light_refraction_coefficient": 1.1 + 0.23 * f / (n - 1)})
    assert all(E.feature_bits(fr) == 4 for fr in frames)
    assert len({fr.planes[0]["params"].light_refraction_coefficient for fr in frames}) == n
    same_as_oracle_per_frame(frames)


R_LIMITS = [0.9, 1.2, 0.0, 1.05, 0.75]


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12"])
def test_r_limit_moves_and_one_frame_has_none(fmt):
    """r_limit_sq > 0 is a run-time test in this flavour: frame 2 has no limit, between frames that have one"""
    n = len(R_LIMITS)
    frames = clip(fmt, n, lambda f: zoom_lens(f, n, r_limit=R_LIMITS[f]), fov=lambda f: 1.6)
    got = same_as_oracle_per_frame(frames, what=fmt)
    # (the limit bites: frame 4's tighter limit leaves background where frame 2, which has none, has picture)
    assert not np.array_equal(got[2][0], got[4][0])


def mesh_of_frame(f, with_fpd, with_mesh, w=W, h=H):
    """synthetic_mesh with its coefficients scaled by the frame index: the cubic terms of the mesh rows and the focal-plane-distortion terms"""
    m = synthetic_mesh(w, h, with_fpd, with_mesh).copy()
    s = np.float32(1.0 + 0.5 * f)
    o = int(m[0])
    if with_mesh:
        n, base = 9, 9 + 9 * 9 * 2
        for comp in range(2):
            for j in range(n):
                rb = base + comp * n * n * 4 + j * n * 4
                m[rb + 2 * n:rb + 4 * n] *= s
    if with_fpd:
        m[o + 4:o + 20] *= s
    return m


@pytest.mark.parametrize("fmt", ["NV12", "YUV422P16LE"])
@pytest.mark.parametrize("with_mesh,with_fpd,inverted", [(True, False, False), (True, True, False), (True, True, True), (False, True, False)])
def test_a_different_mesh_on_every_frame(fmt, with_mesh, with_fpd, inverted):
    n = 5
    frames = clip(fmt, n, lambda f: zoom_lens(f, n), flags=abi.FLAG_FRAMEBUFFER_INVERTED if inverted else 0)
    meshes = [mesh_of_frame(f, with_fpd, with_mesh) for f in range(n)]
    assert all(E.feature_bits(fr, meshes[f]) == 32 for f, fr in enumerate(frames))
    assert len({m.tobytes() for m in meshes}) == n
    same_as_oracle_per_frame(frames, meshes, what="%s mesh %d fpd %d inverted %d" % (fmt, with_mesh, with_fpd, inverted))


def test_the_flavour_reads_each_frames_own_lens_slot():
    """the control: the same launch with every frame given frame 0's LENS slot is NOT the oracle's for the frames that moved, and is the oracle's for frame 0"""
    n = 4
    frames = clip("NV12", n, lambda f: zoom_lens(f, n), t2=moving_centre)
    got = same_as_oracle_per_frame(frames)
    wrong = EL.run_frames_pl(frames, lens_of=lambda f: 0)
    assert all(np.array_equal(a, b) for a, b in zip(oracle(frames[0]), wrong[0]))
    for f in range(1, n):
        assert not np.array_equal(got[f][0], wrong[f][0]), f


def test_the_flavour_reads_each_frames_own_mesh():
    """the same control for the mesh: every frame given frame 0's mesh"""
    n = 4
    frames = clip("NV12", n, lambda f: S.gopro_style_lens(W, H))
    meshes = [mesh_of_frame(f, True, True) for f in range(n)]
    got = same_as_oracle_per_frame(frames, meshes)
    wrong = EL.run_frames_pl(frames, meshes, mesh_of=lambda f: 0)
    assert all(np.array_equal(a, b) for a, b in zip(oracle(frames[0], meshes[0]), wrong[0]))
    for f in range(1, n):
        assert not np.array_equal(got[f][0], wrong[f][0]), f


# ---- a seeded sweep: random clips from the families fused_eligible serves ------------------------------------------------------------------------------------
SWEEP_FORMATS = ["NV12", "P010LE", "YUV420P", "YUV422P16LE", "YUV444P16LE", "RGBA", "RGBAF32", "RGBAF16"]
SWEEP_MODELS = ["opencv_fisheye", "gopro", "sony", "generic_polynomial"]
SWEEP_SEEDS = 8


def sweep_clip(seed):
    """one launch of 3-6 frames: a lens model, format, sampler, shutter direction and readout per seed; the lens (f, c, the model's k), fov, zoom centre per frame;
    odd seeds carry a mesh per frame (the fused kernel serves a mesh without input_rotation: none is drawn)"""
    rng = np.random.default_rng(0x1E55 + seed)
    w, h = [(160, 96), (192, 128), (256, 144)][int(rng.integers(0, 3))]
    model = SWEEP_MODELS[seed % 4]
    fmt, interp = SWEEP_FORMATS[seed % 8], (2, 4, 8)[seed % 3]
    hrs = bool(rng.integers(0, 2))
    readout = float(rng.uniform(-30.0, 30.0))
    n = int(rng.integers(3, 7))
    base = S.gopro_style_lens(w, h) if model == "opencv_fisheye" else dict(lens_for(model, w, h))
    df, dc, dk = float(rng.uniform(-0.04, 0.04)), rng.uniform(-1.5, 1.5, 2), float(rng.uniform(-0.05, 0.05))
    fov0, dfov = float(rng.uniform(0.9, 1.8)), float(rng.uniform(-0.03, 0.03))
    frames = []
    for f in range(n):
        lens = dict(base)
        lens["f"] = tuple(v * (1.0 + df * f) for v in base["f"])
        lens["c"] = (base["c"][0] + float(dc[0]) * f, base["c"][1] + float(dc[1]) * f)
        lens["k"] = [v if v in (0.0, 1.0) else v * (1.0 + dk * f) for v in base["k"]]
        frames.append(S.SyntheticFrame(fmt, w, h, seed=0x5EED + 13 * seed + f, timestamp_ms=1000.0 + 33.3 * f, lens=lens, fov=fov0 + dfov * f, readout_ms=readout,
                                       horizontal_rs=hrs, interpolation=interp, base_overrides={"translation2d": (float(dc[1]) * f, float(dc[0]) * f)},
                                       background_rgba=(0.3, 0.6, 0.1, 1.0)))
    meshes = [mesh_of_frame(f, bool(seed & 2), True, w, h) for f in range(n)] if seed & 1 else None
    return frames, meshes, "%s %dx%d %s interp %d %s readout %.1f, %d frames%s" % (model, w, h, fmt, interp, "hrs" if hrs else "vrs", readout, n, ", meshes" if meshes else "")


@pytest.mark.parametrize("seed", range(SWEEP_SEEDS))
def test_random_moving_lens_clip_is_exact(seed):
    frames, meshes, what = sweep_clip(seed)
    assert all(E.fused_eligible(fr) for fr in frames), what               # (every drawn clip runs: the generator draws from what the fused kernel serves)
    same_as_oracle_per_frame(frames, meshes, what=what)


def test_the_sweep_covers_every_family():
    seen = [sweep_clip(s) for s in range(SWEEP_SEEDS)]
    assert {frames[0].lens["model"] for frames, _, _ in seen} == set(SWEEP_MODELS)
    assert {frames[0].fmt for frames, _, _ in seen} == set(SWEEP_FORMATS)
    assert {frames[0].planes[0]["params"].interpolation for frames, _, _ in seen} == {2, 4, 8}
    assert sum(1 for _, meshes, _ in seen if meshes) == 4
