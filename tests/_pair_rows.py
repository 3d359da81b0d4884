"""The matrix row of every output pixel, from the oracle: what the fused kernel's first pass must arrive at (cpu_undistort.rs: the mid row's projection, rounded,
clamped to the frame and then to the table).  Shared by the pair-row tests and tools/pair_rows_count.py.  Test infrastructure only."""
import numpy as np

from gyroflow_amd import abi, synthetic as S
import _oracle as O

NONE_BITS = 0x7FC0DEAD          # a NaN pattern: where the first pass's projection is None the map keeps it


def pixel_rows(frame, plane=0, clamped=True):
    """int32 [out_h][out_w]: the row of the matrix table each output pixel of ``plane`` is projected with.  The oracle's STMap restatement run with the mid row as a
    one-row table is rotate_and_distort((x, y), matrix_count / 2) per pixel, the first pass itself; the rounding and the two clamps are restated here.
    ``clamped=False``: the rounded first-pass coordinate before either clamp."""
    p = frame.planes[plane]["params"]
    mc = int(p.matrix_count)
    ow, oh = frame.planes[plane]["out_size"][:2]
    assert p.translation2d[0] == 0.0 and p.translation2d[1] == 0.0, "the map starts from (x, y): no translation"
    hrs = bool(p.flags & abi.FLAG_HORIZONTAL_RS)
    start = np.broadcast_to(np.arange(ow, dtype=np.float64)[None, :] if hrs else np.arange(oh, dtype=np.float64)[:, None], (oh, ow))
    if mc > 1:
        q = p.copy()
        q.matrix_count = 1
        mid = np.ascontiguousarray(frame.matrices[mc // 2:mc // 2 + 1], dtype=np.float32)
        pt = O.stmap_undistort(q, frame.model, frame.digital, mid, ow, oh, fill=NONE_BITS)
        v = pt[:, :, 0 if hrs else 1].astype(np.float64)
        none = pt.view(np.uint32)[:, :, 0] == NONE_BITS
        v = np.where(none, start, v)
    else:
        v = start
    r = np.sign(v) * np.floor(np.abs(v) + 0.5)                      # roundf: halves away from zero (exact in f64 for every f32)
    if not clamped:
        return np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    r = np.clip(r, 0.0, float(p.width if hrs else p.height))       # ... clamped to the frame
    return np.minimum(r, float(mc - 1)).astype(np.int32)            # ... and to the table


def pair_shares(rows, wave_px=128, quad_px=8):
    """-> (share of pixel pairs (2k, 2k + 1) of a line whose rows differ, share of 4-lane groups, share of waves that hold such a pair).  A wave's lane-row is
    ``wave_px`` consecutive pixels of one line from a multiple of ``wave_px``, a 4-lane group ``quad_px`` of them; a partial last group counts as one."""
    h, w = rows.shape
    w2 = w // 2 * 2
    d = rows[:, 0:w2:2] != rows[:, 1:w2:2]

    def groups(per):
        n = -(-d.shape[1] // per)
        pad = np.zeros((h, n * per), dtype=bool)
        pad[:, :d.shape[1]] = d
        return pad.reshape(h, n, per).any(axis=2)
    return float(d.mean()), float(groups(quad_px // 2).mean()), float(groups(wave_px // 2).mean())


# ---- the clips of the pair-row tests (tests/test_emu_pair_rows.py, tests/test_gpu_pair_rows.py): each a regime of "the pair's two rows differ" ----------------

def set_row_rotations(fr, fov, euler_of):
    """Replace the frame's matrix table (gyroflow_amd.synthetic.row_matrices' form: inv(new_k * R_row), the same sign flips): row y turns by
    euler_of(t) = (yaw, pitch, roll) in degrees, t = (y - rows / 2) / rows — t = 0 is the row the first pass projects with."""
    rows = fr.matrices.shape[0]
    nk = S.new_k(fr.lens, fov, fr.out_size[0], fr.out_size[1])
    out = np.zeros((rows, 14), dtype=np.float32)
    for y in range(rows):
        r = S.quat_to_matrix(S.quat_from_euler_deg(*euler_of((y - rows // 2) / float(rows))))
        r[0, 1] *= -1.0; r[0, 2] *= -1.0
        r[1, 0] *= -1.0; r[2, 0] *= -1.0
        out[y, :9] = np.linalg.inv(nk @ r).reshape(9).astype(np.float32)
    fr.matrices = out
    return fr


def long_lens(w, h, times, k=(0.0, 0.0, 0.0, 0.0)):
    return {"model": "opencv_fisheye", "f": (times * w, times * w), "c": (w / 2.0, h / 2.0), "k": list(k) + [0.0] * 8, "r_limit": 0.0}


CLAMP_TILT_DEG = 20.0         # (the sign that moves the first pass DOWN the source: the tests that use it assert where it lands)


def case_frame(case, fmt, w, h, f=0, interp=2, fov=None, lens=None, pixels=True):
    """frame f of the clip of one case:
    single  no rolling shutter: one matrix, the comparison folds
    flat    rolling shutter (pitch alone, +-4 px over the frame), no roll, a centre crop (half the source each way) through a lens of 200 source widths with no
            distortion: the first pass is y + h / 2 to a thousandth of a pixel, no pair differs
    roll    25 degrees of roll (+ f) in the first pass's row, yaw / pitch / roll moving down the frame (a 30 ms readout of a fast pan): sin 25 deg of the pairs differ
    hrs     horizontal rolling shutter: the row follows x, through a lens of two widths at fov 1.05 nearly every pair differs
    clamp   8 degrees of roll and a tilt of the first pass's row that carries it past the table's last row over the lower part of the frame
    """
    seed, ts = 0x3A70 + 17 * f, 1000.0 + 33.3 * f
    kw = dict(seed=seed, timestamp_ms=ts, interpolation=interp, pixels=pixels)
    if case == "single":
        return S.SyntheticFrame(fmt, w, h, readout_ms=0.0, fov=fov or 1.0, lens=lens, **kw)
    if case == "flat":
        fr = S.SyntheticFrame(fmt, 2 * w, 2 * h, out_size=(w, h), readout_ms=30.0, fov=1.0, lens=long_lens(2 * w, 2 * h, 100.0), **kw)
        per_px = float(np.degrees(1.0 / fr.lens["f"][0]))
        return set_row_rotations(fr, 1.0, lambda t: (0.0, (8.0 + f) * per_px * t, 0.0))
    if case == "hrs":
        fr = S.SyntheticFrame(fmt, w, h, readout_ms=30.0, fov=1.05, horizontal_rs=True, lens=long_lens(w, h, 2.0, (0.03, 0.01, -0.01, 0.002)), **kw)
        return set_row_rotations(fr, 1.05, lambda t: (1.5 * t, -1.0 * t + 0.1 * f, 0.8 * t))
    if case == "roll":
        fov = fov or 1.0
        fr = S.SyntheticFrame(fmt, w, h, readout_ms=30.0, fov=fov, lens=lens, **kw)
        return set_row_rotations(fr, fov, lambda t: (3.0 * t + 0.5, 4.0 * t - 0.3 * f, 25.0 + f + 6.0 * t))
    if case == "clamp":
        fr = S.SyntheticFrame(fmt, w, h, readout_ms=30.0, fov=1.0, **kw)
        return set_row_rotations(fr, 1.0, lambda t: (2.0 * t, CLAMP_TILT_DEG + 5.0 * t, 8.0 + f))
    raise KeyError(case)


def clip_shares(frames):
    """-> per frame (pairs, 4-lane groups, waves) of :func:`pair_shares` on the luma plane's rows"""
    return [pair_shares(pixel_rows(fr)) for fr in frames]
