"""Host statement of the adaptive-zoom fov search (src/core/zooming/) — the checker of gfw_zoom_fovs / gfw_zoom_smooth.  Test
infrastructure: written from the cited Rust, independent of the device code; not part of the product package.

  points_around_rect   fov_iterative.rs:154-175   numpy.float32 scalar operations in the reference's order
  interpolate_points   fov_iterative.rs:180-188
  nearest_edge         fov_iterative.rs:136-151   the sequential fold
  find_fov             fov_iterative.rs:91-134    the loop `for _ in 1..5` AS WRITTEN (see its docstring)
  point_rotations      frame_transform.rs:376-410 (at_timestamp_for_points) in float64 over sampled tracks (_hoststmt.quat_at)
  map_points           cpu_undistort.rs:636-641   = the oracle's undistort_points with one rotation per point
  zoom_smooth          zooming/mod.rs:55-68, zoom_dynamic.rs:56-194, fov_iterative.rs:59-69 in Python floats (math.exp is glibc's)

No reference-produced vector exists for this path (the Rust crate cannot be built here, the OpenCL twin has no zoom search), so
tests/test_zoom_statement.py holds this statement against what the search is for — a frame rendered at 0.97 x fov_minimal shows no
background, at 1.03 x it does — before anything is compared with it.
"""
import math

import numpy as np

from gyroflow_amd import abi, synthetic as S
import _hoststmt as H
import _oracle as O

f32 = np.float32
RECT_POINTS = 120


# ------------------------------------------------------------------------------------------------ fov_iterative.rs
def points_around_rect(w, h, margin, w_div=31, h_div=31):
    """:154-175.  w, h, margin: f32."""
    w = f32(f32(w) - f32(f32(margin) * f32(2.0)))
    h = f32(f32(h) - f32(f32(margin) * f32(2.0)))
    wcnt, hcnt = max(w_div, 2) - 1, max(h_div, 2) - 1
    wstep, hstep = f32(w / f32(wcnt)), f32(h / f32(hcnt))
    p = []
    for i in range(wcnt):
        p.append((f32(f32(i) * wstep), f32(0.0)))
    for i in range(hcnt):
        p.append((w, f32(f32(i) * hstep)))
    for i in range(wcnt):
        p.append((f32(f32(wcnt - i) * wstep), h))
    for i in range(hcnt):
        p.append((f32(0.0), f32(f32(hcnt - i) * hstep)))
    return [(f32(x + f32(margin)), f32(y + f32(margin))) for x, y in p]


def interpolate_points(pts, steps):
    """:180-188"""
    d = steps + 1
    new_len = d * len(pts) - steps
    out = []
    for i in range(new_len):
        idx1 = i // d
        idx2 = min(idx1 + 1, len(pts) - 1)
        f = f32(f32(i % d) / f32(d))
        out.append((f32(pts[idx1][0] + f32(f * f32(pts[idx2][0] - pts[idx1][0]))), f32(pts[idx1][1] + f32(f * f32(pts[idx2][1] - pts[idx1][1])))))
    return out


def nearest_edge(polygon, center, initial, inv_aspect):
    """:136-151 -> (Option<usize> as int or None, (f32, f32))"""
    idx, mp = None, initial
    with np.errstate(all="ignore"):
        for i, (x, y) in enumerate(polygon):
            ap = (f32(abs(f32(x - center[0]))), f32(abs(f32(y - center[1]))))
            if ap[0] < mp[0] and ap[1] < mp[1]:
                if ap[1] > f32(ap[0] * inv_aspect):
                    idx, mp = i, (f32(ap[1] / inv_aspect), ap[1])
                else:
                    idx, mp = i, (ap[0], f32(ap[0] * inv_aspect))
    return idx, mp


USIZE_MAX = 2 ** 64 - 1


def find_fov(map_points, width, height, org_output_size, margin, zoom_center, trace=None):
    """FovIterative::new (:71-89) + find_fov (:91-134).  map_points(k, pts) = undistort_points_with_rolling_shutter of the k-th point set of the
    frame (k = 0 the outline, k >= 1 the k-th refinement) -> [(f32, f32)].  -> (fov f64, debug polygon [120][2] f64).

    The loop is restated as written:
      * `rect[idx]`: idx is the index into the polygon folded last — the 63-point refined polygon from the second round on — yet indexes the 120 outline points;
      * `idx.overflowing_sub(1).0 % len` is usize::MAX % 120 = 15 for idx = 0 (the same with a 32-bit usize), not 119;
      * a round whose second fold returns None leaves nearest.0 = None; the next round folds the OLD refined polygon once more and breaks.
    trace: optional list, gets one (round, idx of the first fold, idx of the second fold) per round that refined."""
    ratio = f32(f32(width) / f32(max(org_output_size[0], 1)))
    input_dim = (f32(width), f32(height))
    output_dim = (f32(f32(org_output_size[0]) * ratio), f32(f32(org_output_size[1]) * ratio))
    with np.errstate(all="ignore"):
        inv_aspect = f32(output_dim[1] / output_dim[0])
    rect = points_around_rect(input_dim[0], input_dim[1], f32(margin))
    center = (f32(input_dim[0] / f32(2.0)), f32(input_dim[1] / f32(2.0)))
    off = (f32(f32(zoom_center[0]) * input_dim[0]), f32(f32(zoom_center[1]) * input_dim[1]))

    def undistort(k, pts):
        with np.errstate(all="ignore"):
            return [(f32(f32(x) - off[0]), f32(f32(y) - off[1])) for x, y in map_points(k, pts)]          # :99-102

    polygon = undistort(0, rect)
    with np.errstate(all="ignore"):
        debug = np.array([[float(f32(x / input_dim[0])), float(f32(y / input_dim[1]))] for x, y in polygon], dtype=np.float64)      # :103-105
    initial = (f32(1000000.0), f32(f32(1000000.0) * inv_aspect))
    nearest = (None, initial)
    for rnd in range(1, 5):
        nearest = nearest_edge(polygon, center, nearest[1], inv_aspect)
        if nearest[0] is not None:
            idx = nearest[0]
            ln = len(rect)
            relevant = [rect[((idx - 1) if idx >= 1 else USIZE_MAX) % ln], rect[idx], rect[(idx + 1) % ln]]
            distorted = interpolate_points(relevant, 30)
            polygon = undistort(rnd, distorted)
            nearest = nearest_edge(polygon, center, nearest[1], inv_aspect)
            if trace is not None:
                trace.append((rnd, idx, nearest[0]))
        else:
            break
    with np.errstate(all="ignore"):
        return float(f32(f32(nearest[1][0] * f32(2.0)) / output_dim[0])), debug


# ------------------------------------------------------------------------------------------------ statement clips
# coefficients of the nine physical lens models (the values tests/test_gpu_lens_models.py renders with)
PHYSICAL = {
    "opencv_fisheye": [0.045, 0.02, -0.02, 0.006],
    "opencv_standard": [0.12, -0.05, 0.001, 0.002, 0.01, 0.02, -0.01, 0.001, 0.0005, -0.0002, 0.0003, 0.0001],
    "poly3": [0.06],
    "poly5": [0.08, -0.02],
    "ptlens": [0.01, -0.03, 0.02],
    "insta360": [0.05, -0.01, 0.002, 0.001, -0.001, 0.6],
    "sony": [1.0, 0.01, -0.05, 0.02, 0.003, -0.001],
    "generic_polynomial": [1.0, 0.01, -0.05, 0.02, 0.003, -0.001, 0.0005, 0.0, 0.0, 0.0, 0.0, 0.0],
    "gopro": [0.0, 1.0, 0.01, -0.12, 0.02, 0.01, -0.004],
}
_TRACKS = {}


def _track(seed, t0, t1, scale):
    """synthetic.sampled_track at 1 kHz, kept per (seed, range, scale): most clips share theirs"""
    key = (seed, t0, t1, scale)
    if key not in _TRACKS:
        _TRACKS[key] = S.sampled_track(seed, t0, t1, scale=scale)
    return _TRACKS[key]


class Clip:
    """One clip of the zoom search: lens, sizes, readout, the values of the frames' descriptors, sampled tracks, frame times.  keyframed: the zoom centre, the
    lens-correction strength and the per-frame time offset differ from frame to frame (fov_iterative.rs:41-57, per_frame_time_offsets), and the clip has gyro / video
    sync offsets (gyro_source/mod.rs:884-908)."""

    def __init__(self, name, lens=None, size=(320, 180), out=(320, 180), readout=0.0, horizontal=False, lca=1.0, center=(0.0, 0.0), margin=0.0,
                 video_rotation=0.0, suppress=False, refraction=1.0, digital=None, digital_params=(), track_scale=1.0, seed=11, frames=24, keyframed=False):
        self.name, self.size, self.out = name, tuple(size), tuple(out)
        self.lens = dict(lens) if lens is not None else S.gopro_style_lens(*size)
        if digital:
            self.lens["digital"] = digital
        self.readout, self.horizontal, self.lca, self.center, self.margin = float(readout), horizontal, float(lca), tuple(center), float(margin)
        self.video_rotation, self.suppress, self.refraction = float(video_rotation), bool(suppress), float(refraction)
        self.digital_params, self.track_scale, self.seed = list(digital_params), track_scale, seed
        self.timestamps = [1000.0 + 130.0 * k for k in range(frames)]
        self.fov = 1.0                                               # get_fov(use_fovs = false) on the patched params: 1.0 * width / width
        self.keyframed = keyframed
        # (timestamps_us, offsets_ms) of the sync points and the duration, or None: no offsets, a positive duration
        self.sync_offsets = (np.array([900000, 2500000, 4300000], dtype=np.int64), np.array([2.0, -1.5, 3.25])) if keyframed else None
        self.duration_ms = 5000.0 if keyframed else 1.0

    @property
    def model(self):
        return abi.MODELS[self.lens["model"]]

    @property
    def digital(self):
        return abi.MODELS[self.lens.get("digital", "none")]

    def lca_at(self, k):
        return self.lca - 0.08 * (k % 5) if self.keyframed else self.lca

    def center_at(self, k):
        return (self.center[0] + 0.01 * ((k % 7) - 3), self.center[1] - 0.008 * ((k % 4) - 1)) if self.keyframed else self.center

    def time_offset_at(self, k):
        """file_metadata.per_frame_time_offsets[frame], ms"""
        return 0.75 * ((k % 3) - 1) + 0.125 * k if self.keyframed else 0.0

    @property
    def tracks(self):
        """(org, smoothed): (timestamps_us, quaternions) at 1 kHz around the clip; the smoothed one a low-amplitude track of another seed"""
        t0, t1 = self.timestamps[0] - 200.0, self.timestamps[-1] + 200.0
        return _track(self.seed, t0, t1, self.track_scale), _track(self.seed + 7777, t0, t1, 0.25 * self.track_scale)

    def quat_at(self, track, timestamp_ms):
        return H.quat_at(track[0], track[1], timestamp_ms, self.sync_offsets, self.duration_ms)

    def new_k(self):
        return S.new_k(self.lens, self.fov, self.size[0], self.size[1])           # mod.rs:47-49: output size = source size

    def kernel_params(self, k=0):
        """the KernelParams undistort_points builds for frame k (cpu_undistort.rs:671-683) + what its lens-correction branch reads (amount, fov)"""
        kp = S.base_kernel_params(self.lens, self.fov, 1, lens_correction_amount=self.lca_at(k), digital_lens_params=self.digital_params,
                                  light_refraction_coefficient=self.refraction)
        kp.width, kp.height, kp.output_width, kp.output_height = self.size[0], self.size[1], self.size[0], self.size[1]
        return kp


def physical_lens(model, size):
    lens = S.gopro_style_lens(*size)
    lens["model"] = model
    lens["k"] = PHYSICAL[model] + [0.0] * (12 - len(PHYSICAL[model]))
    if model == "gopro":
        lens["r_limit"] = 2.5
    return lens


def statement_clips():
    clips = []
    for out in ((320, 180), (240, 180)):
        for readout in (0.0, 12.0):
            for lca in (1.0, 0.6):
                for cz in ((0.0, 0.0), (0.04, -0.03)):
                    clips.append(Clip("fisheye-%dx%d-r%g-l%g-c%g" % (out[0], out[1], readout, lca, cz[0]), out=out, readout=readout, lca=lca, center=cz))
    for model in sorted(PHYSICAL):
        clips.append(Clip("%s-r0-l1" % model, lens=physical_lens(model, (320, 180)), seed=13))
        clips.append(Clip("%s-r12-l0.6" % model, lens=physical_lens(model, (320, 180)), readout=12.0, lca=0.6, center=(0.04, -0.03), out=(240, 180), seed=13))
    clips.append(Clip("readout-neg", readout=-12.0))
    clips.append(Clip("readout-horizontal", readout=12.0, horizontal=True))
    clips.append(Clip("track-scale3", readout=12.0, track_scale=3.0))
    clips.append(Clip("digital-lens", digital="gopro_superview", digital_params=[], lca=0.6))
    clips.append(Clip("refraction", refraction=1.33))
    clips.append(Clip("margin2", margin=2.0, readout=12.0))
    clips.append(Clip("rotation90", video_rotation=90.0, out=(180, 320)))
    clips.append(Clip("suppress", suppress=True, readout=12.0))
    clips.append(Clip("keyframed", readout=12.0, lca=0.9, center=(0.01, -0.01), out=(240, 180), keyframed=True))     # every frame its own centre, strength and time offset; sync offsets
    return clips


# ------------------------------------------------------------------------------------------------ frame_transform.rs:376-410
def point_rotations(clip, pts, k):
    """at_timestamp_for_points for frame k: `new_k * R` per point ([n][9] f32; ONE row when the frame readout time is zero), float64 over the clip's tracks."""
    org, smoothed = clip.tracks
    frt = clip.readout
    w, h = clip.size
    row_readout_time = frt / float(w if clip.horizontal else h)
    ts = clip.timestamps[k] + clip.time_offset_at(k)                                                   # :385 per_frame_time_offsets
    start_ts = ts - (frt / 2.0)
    a = clip.video_rotation * (math.pi / 180.0)
    image_rotation = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
    nk = clip.new_k()
    q1 = clip.quat_at(org, ts)
    q1 = np.array([q1[0], -q1[1], -q1[2], -q1[3]]) / np.dot(q1, q1)                                    # inverse()
    pre = S.quat_mul(clip.quat_at(smoothed, ts), q1)                                                   # smoothed_quat1 * quat1
    out = []
    for x, y in (pts if abs(frt) > 0.0 else [(0.0, 0.0)]):
        quat_time = start_ts + row_readout_time * float(x if clip.horizontal else y) if abs(frt) > 0.0 else start_ts
        q = S.quat_mul(pre, clip.quat_at(org, quat_time))
        rq = S.quat_to_matrix(q)
        r = [[sum(image_rotation[i][m] * float(rq[m][j]) for m in range(3)) for j in range(3)] for i in range(3)] if clip.video_rotation != 0.0 else [[float(v) for v in row] for row in rq]
        r[0][1] *= -1.0; r[0][2] *= -1.0                                                               # :402-403: always these four
        r[1][0] *= -1.0; r[2][0] *= -1.0
        if clip.suppress:
            r = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        out.append([f32((float(nk[i][0]) * r[0][j] + float(nk[i][1]) * r[1][j]) + float(nk[i][2]) * r[2][j]) for i in range(3) for j in range(3)])
    return np.array(out, dtype=np.float32)


def mapper_for(clip, k, rotation=None, perturb=None):
    """map_points of frame k.  rotation: None = rotations from the tracks; or 9 f32 = the frame's one caller-given `new_k * R` (readout must be 0).
    perturb: None or a numpy Generator — the sensitivity measurement: every entry of every f32 rotation the DEVICE derives with its own acos / sin moves by a random
    -2 .. +2 ULP.  A frame without rolling shutter has ONE rotation, displaced once for the outline and the refinement alike; under suppress_rotation the rotation is
    new_k alone, exact on either side, and stays."""
    kp = clip.kernel_params(k)
    cache = {}
    if perturb is not None and clip.suppress:
        perturb = None
    once = perturb.integers(-2, 3, (1, 9)).astype(np.int32) if perturb is not None and clip.readout == 0.0 else None

    def map_points(pass_index, pts):
        arr = np.array(pts, dtype=np.float32).reshape(-1, 2)
        if rotation is not None:
            assert clip.readout == 0.0
            rot = np.repeat(np.asarray(rotation, dtype=np.float32).reshape(1, 9), len(arr), 0)
        else:
            key = arr.tobytes()
            if key not in cache:
                cache[key] = point_rotations(clip, pts, k)
            rot = cache[key]
            if rot.shape[0] == 1:
                rot = np.repeat(rot, len(arr), 0)
        if perturb is not None:
            delta = once if once is not None else perturb.integers(-2, 3, rot.shape).astype(np.int32)
            rot = np.where(rot == 0.0, rot, (rot.view(np.int32) + delta).view(np.float32))            # (an exact zero is a product with an exact zero)
        o = O.undistort_points(kp, clip.model, clip.digital, np.ascontiguousarray(rot), points=arr, index_mode=abi.POINT_INDEX_PER_POINT)
        return [(f32(x), f32(y)) for x, y in o]
    return map_points


def frame_rotation(clip, k):
    """the one `new_k * R` of frame k without rolling shutter, as the statement derives it from the tracks (what a caller hands to gfw_zoom_fovs as `rotations`)"""
    saved = clip.readout
    clip.readout = 0.0
    try:
        return point_rotations(clip, [(0.0, 0.0)], k)[0]
    finally:
        clip.readout = saved


def frame_fov(clip, k, rotation=None, perturb=None, trace=None):
    """find_fov of frame k -> (fov f64, debug polygon [120][2])"""
    return find_fov(mapper_for(clip, k, rotation, perturb), clip.size[0], clip.size[1], clip.out, clip.margin, clip.center_at(k), trace)


def clip_fovs(clip, given_rotations=False, perturb=None, trace=None):
    """find_fov of every frame -> (fov_minimal [n] f64, debug polygons [n][120][2] f64)."""
    fovs, dbg = [], []
    for k in range(len(clip.timestamps)):
        tr = [] if trace is not None else None
        f, d = frame_fov(clip, k, frame_rotation(clip, k) if given_rotations else None, perturb, tr)
        fovs.append(f)
        dbg.append(d)
        if trace is not None:
            trace.append(tr)
    return np.array(fovs, dtype=np.float64), np.array(dbg, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ zooming/mod.rs:55-68, zoom_dynamic.rs
def _as_usize(v):
    if v != v or v <= 0.0:
        return 0
    return int(min(v, 2.0 ** 64 - 1))


def pad_edge(arr, before, after):                      # zoom_dynamic.rs:119-131
    first = arr[0] if arr else 0.0
    last = arr[-1] if arr else 0.0
    return [first] * before + list(arr) + [last] * after


def _fmin(a, b):                                       # f64::min: the non-NaN operand wins
    if a != a:
        return b
    if b != b:
        return a
    return b if b < a else a


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return b if b > a else a


def envelope_follower(a, alpha):                       # :170-194 with a constant alpha
    if not a:
        return []
    q = a[-1]
    smoothed_rev = []
    for x in reversed(a):
        q = _fmin(x, x * alpha + q * (1.0 - alpha))
        smoothed_rev.append(q)
    q = smoothed_rev[-1]
    out = []
    for x in reversed(smoothed_rev):
        q = _fmin(x, x * alpha + q * (1.0 - alpha))
        out.append(q)
    return out


def zoom_smooth(fov_minimal, window, scaled_fps, method=0, trim_ranges=()):
    """fov_iterative.rs:59-69 (trim ranges), then mod.rs:55-68 -> (fovs, fov_minimal after the trim ranges), lists of Python floats."""
    v = [float(x) for x in fov_minimal]
    n = len(v)
    if n == 0:
        return [], []
    if len(trim_ranges):
        l = float(n - 1)
        max_fov = v[0]
        for x in v[1:]:
            max_fov = _fmax(max_fov, x)
        for i in range(n):
            if not any(i >= _as_usize(math.floor(l * r0)) and i <= _as_usize(math.ceil(l * r1)) for r0, r1 in trim_ranges):
                v[i] = max_fov
    minimal = list(v)
    if window < -0.9:                                  # static zoom
        m = v[0]
        for x in v[1:]:
            m = _fmin(m, x)
        return [m] * n, minimal
    if window > 0.0001:                                # dynamic zoom (static window)
        if method == 1:
            first_pass_alpha = 1.0 - math.exp(-(1.0 / scaled_fps) / window)
            second_pass_alpha = 1.0 - math.exp(-(1.0 / scaled_fps) / 0.2)
            return envelope_follower(envelope_follower(v, first_pass_alpha), second_pass_alpha), minimal
        frames = _as_usize(math.floor(window * scaled_fps))                      # get_frames_per_window
        if frames % 2 == 0:
            frames += 1
        pad = pad_edge(v, frames // 2, frames // 2)
        fov_min = []
        for i in range(len(pad) - frames + 1):                                   # min_rolling: a.windows(window)
            m = pad[i]
            for x in pad[i + 1:i + frames]:
                m = _fmin(m, x)
            fov_min.append(m)
        fov_min_pad = pad_edge(fov_min, frames // 2, frames // 2)
        std = frames / 6.0
        sig2 = 2.0 * (std * std)
        g = [math.exp(-float(x * x) / sig2) for x in range(-(frames // 2), frames // 2 + 1)]        # gaussian_window
        total = 0.0
        for x in g:
            total += x
        g = [x / total for x in g]
        out = []
        for i in range(len(fov_min_pad) - frames + 1):                           # convolve
            s = 0.0
            for x, y in zip(fov_min_pad[i:i + frames], g):
                s += x * y
            out.append(s)
        return out, minimal
    return [1.0] * n, minimal                          # disabled zoom
