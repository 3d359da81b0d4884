"""Seeded random clips for gfw_undistort_clip_params: a lens per clip, KernelParams that move per frame as an adaptive-zoom render moves them (fov drifting by
up to 0.03 per frame from a start in [0.6, 2.2], the zoom centre starting within 5 % of the frame size and drifting by up to 1 % of it per frame, the render
loop's fill flag on about one frame in ten).  Shared by the CPU tier (tests/test_emu_clip_params.py, through the interpreted kernel) and the GPU tier
(tests/test_gpu_clip_params_cover.py), which also asks the library on the CPU tier which of its clips the host certifies (gfw_debug_jit_key_clip_params)."""
import numpy as np

from gyroflow_amd import abi, synthetic as S
from _shapes import lens_for

SIZES = [(320, 180), (640, 360), (960, 540), (1280, 720), (1920, 1080)]          # tests/test_gpu_pass1_sweep.py SIZES
SWEEP_MODELS = ["opencv_fisheye", "opencv_fisheye", "gopro", "sony", "generic_polynomial"]


def fisheye_lens(rng, w, h):
    """a fisheye lens as tests/test_emu_pass1_audit.py random_clip draws it: f 0.3-1.2 w, principal point within 5 % of the centre, k0..k3"""
    lens = S.gopro_style_lens(w, h)
    lens["f"] = (float(rng.uniform(0.3, 1.2)) * w,) * 2
    lens["c"] = (w / 2.0 + float(rng.uniform(-0.05, 0.05)) * w, h / 2.0 + float(rng.uniform(-0.05, 0.05)) * h)
    lens["k"] = [float(rng.uniform(-0.08, 0.12)), float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-0.03, 0.03)), float(rng.uniform(-0.01, 0.01))] + [0.0] * 8
    return lens


def motion(rng, n, w, h, fill_rate=0.1):
    """per frame: fov, zoom centre (translation2d), fill flag"""
    fov0, dfov = float(rng.uniform(0.6, 2.2)), float(rng.uniform(-0.03, 0.03))
    c0, dc = rng.uniform(-0.05, 0.05, 2) * (w, h), rng.uniform(-0.01, 0.01, 2) * (w, h)
    fovs = [max(0.5, fov0 + dfov * f) for f in range(n)]
    t2s = [(float(c0[0] + dc[0] * f), float(c0[1] + dc[1] * f)) for f in range(n)]
    fills = [bool(rng.random() < fill_rate) for _ in range(n)]
    return fovs, t2s, fills


def rotate(fr, lens, fov, base, rate, rows):
    """the frame's `rows` per-row matrices (one per source row, or column under a horizontal shutter) for a camera at `base` (radians per axis) turning at `rate`
    (radians over the readout), as tests/test_gpu_pass1_sweep.py random_clip builds them (the same products, every row at once); matrix_count follows"""
    nk = S.new_k(lens, fov, fr.width, fr.height)
    t = (np.arange(rows) / max(rows - 1, 1)) - 0.5
    a = base[None, :] + rate[None, :] * t[:, None]
    cx, sx, cy, sy, cz, sz = np.cos(a[:, 0]), np.sin(a[:, 0]), np.cos(a[:, 1]), np.sin(a[:, 1]), np.cos(a[:, 2]), np.sin(a[:, 2])
    one, zero = np.ones(rows), np.zeros(rows)
    rx = np.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], 1).reshape(rows, 3, 3)
    ry = np.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], 1).reshape(rows, 3, 3)
    rz = np.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], 1).reshape(rows, 3, 3)
    r = rz @ ry @ rx
    r[:, 0, 1] *= -1.0; r[:, 0, 2] *= -1.0; r[:, 1, 0] *= -1.0; r[:, 2, 0] *= -1.0
    m = np.zeros((rows, 14), dtype=np.float32)
    m[:, :9] = np.linalg.inv(np.asarray(nk)[None] @ r).reshape(rows, 9).astype(np.float32)
    fr.matrices = m
    for pl in fr.planes:
        pl["params"].matrix_count = rows


def gpu_clip(i, rng):
    """Clip i of the device audit sweep (seed 0x9F20): the generator above plus a camera rotation up to 15 degrees per axis turning at up to 250 deg/s over
    the readout, a little more each frame; sizes of SIZES, 4K at clips 7, 27, 47 and 8K at clip 57; 4-16 frames.  -> (model name, frames)
    (the frames are made with a single matrix and given their rows here: synthetic.py's per-row loop would take a minute over the sweep)"""
    w, h = (7680, 4320) if i == 57 else (3840, 2160) if i in (7, 27, 47) else SIZES[int(rng.integers(0, len(SIZES)))]
    model = SWEEP_MODELS[int(rng.integers(0, len(SWEEP_MODELS)))]
    lens = fisheye_lens(rng, w, h) if model == "opencv_fisheye" else dict(lens_for(model, w, h))
    n = int(rng.integers(4, 17))
    fmt = "YUV422P16LE" if rng.integers(0, 2) else "NV12"
    hrs = bool(rng.integers(0, 4) == 0)
    readout = float(rng.uniform(-30.0, 30.0))
    if abs(readout) < 0.5:
        readout = 8.0
    base = np.radians(rng.uniform(-15.0, 15.0, 3))
    rate = np.radians(rng.uniform(-250.0, 250.0, 3)) * (readout / 1000.0)
    turn = np.radians(rng.uniform(-0.5, 0.5, 3))
    fovs, t2s, fills = motion(rng, n, w, h)
    frames = []
    for f in range(n):
        fr = S.SyntheticFrame(fmt, w, h, seed=0x9F20 + 97 * i + f, timestamp_ms=1000.0 + 33.3 * f, lens=lens, fov=fovs[f], readout_ms=0.0, horizontal_rs=hrs,
                              base_overrides={"translation2d": t2s[f]}, flags=abi.FLAG_FILL_WITH_BACKGROUND if fills[f] else 0, pixels=False)
        rotate(fr, lens, fovs[f], base + turn * f, rate, w if hrs else h)
        frames.append(fr)
    return model, frames


def gpu_clips():
    """the 60 clips of the device audit sweep, in order (the generator's state runs through them)"""
    rng = np.random.default_rng(0x9F20)
    for i in range(60):
        yield gpu_clip(i, rng)
