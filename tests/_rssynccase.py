"""TEST INFRASTRUCTURE: the planted clips the rs-sync offset search is tested on (statement and device alike).

  plant      an independent float64 path: a camera whose orientation is a smooth sum-of-sines rotation vector and whose position moves at a constant velocity,
             in front of a static scene (x +-4, y +-2.5, z 3 .. 20); a pinhole of 1920 x 1080 at f = 1000 (the project's lens synthetic with k = 0), flow image
             960 x 540, 30 frames a second.  Every point is observed at ITS OWN row time: t = frame + readout * (y / height) with the row iterated to its fixed
             point, at the gyro time t + delay.  The gyro track samples the same orientation at 200 Hz or 1 kHz over 4 s.  Pixels are rounded to f32; `outliers`
             of the second frame's points are displaced by up to +-30 px an axis.
  SHAPES     "gpu": 3 ranges — one without pairs, one of pairs of 0, 1, 2, 63, 64, 65 and 200 points, one whose times run past both ends of the 4 s track;
             radius 30 ms: 21 + 3 x 17 candidates.  "emu": 2 ranges of 3 small pairs, radius 6 ms."""
import numpy as np

from gyroflow_amd import abi
import _posecase as PC
import _posesscase as EC
import _posessstmt as ES
import _rssyncstmt as RS

FPS, FLOW, TRACK_SECONDS = 30.0, (960, 540), 4.0
SIZES_GPU = [0, 1, 2, 63, 64, 65, 200]


def rotvec(t):
    t = np.asarray(t, dtype=np.float64)
    return np.stack([0.10 * np.sin(2 * np.pi * 1.3 * t + 0.3) + 0.04 * np.sin(2 * np.pi * 4.1 * t),
                     0.08 * np.sin(2 * np.pi * 0.9 * t + 1.1) + 0.05 * np.sin(2 * np.pi * 3.3 * t + 0.5),
                     0.06 * np.sin(2 * np.pi * 1.7 * t + 2.0) + 0.03 * np.sin(2 * np.pi * 5.2 * t + 0.9)], axis=-1)


def quat_true(t):
    """(w, x, y, z) [..][4] of the camera's orientation at the gyro time t"""
    rv = rotvec(t)
    th = np.linalg.norm(rv, axis=-1, keepdims=True)
    return np.concatenate([np.cos(th / 2), rv / th * np.sin(th / 2)], axis=-1)


def rot_of(q):
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def track(rate_hz, seconds=TRACK_SECONDS):
    """-> (ts_us int64 [n], wxyz f64 [n][4])"""
    ts = np.round(np.arange(int(seconds * rate_hz) + 1) * (1000000.0 / rate_hz)).astype(np.int64)
    return ts, np.ascontiguousarray(quat_true(ts / 1000000.0))


D = np.array([1.0, -1.0, -1.0])


def observe(X, frame_s, delay_s, readout_s, velocity, K, scale, height):
    """the flow-image pixels of the world points X [n][3] in the frame at frame_s"""
    y = np.full(len(X), height / 2.0)
    for _ in range(8):
        g = frame_s + readout_s * (y / height) + delay_s
        R = rot_of(quat_true(g))
        pc = np.einsum("nji,nj->ni", R, X - g[:, None] * velocity) * D               # cam = D R^T (X - c)
        px = np.stack([pc[:, 0] / pc[:, 2] * K[0, 0] + K[0, 2], pc[:, 1] / pc[:, 2] * K[1, 1] + K[1, 2]], axis=1) * scale
        y = px[:, 1]
    return px


def plant_pair(cam, n, frame_us, next_us, delay_s, readout_ms, velocity, seed, outliers=0.0):
    """-> (ts_a_us, ts_b_us, points_a f32 [n][2], points_b f32 [n][2])"""
    g = np.random.default_rng(seed)
    Xc = np.stack([g.uniform(-4, 4, n), g.uniform(-2.5, 2.5, n), g.uniform(3, 20, n)], axis=1)
    c0 = (frame_us / 1e6 + delay_s) * np.asarray(velocity)
    X = np.einsum("ij,nj->ni", rot_of(quat_true(frame_us / 1e6 + delay_s)), Xc * D) + c0      # in front of the camera at the pair's first frame
    scale = np.array(cam.flow, dtype=np.float64) / np.array(cam.video, dtype=np.float64)
    a = observe(X, frame_us / 1e6, delay_s, readout_ms / 1000.0, np.asarray(velocity), cam.K, scale, float(cam.flow[1])).astype(np.float32)
    b = observe(X, next_us / 1e6, delay_s, readout_ms / 1000.0, np.asarray(velocity), cam.K, scale, float(cam.flow[1])).astype(np.float32)
    bad = g.permutation(n)[:int(outliers * n)]
    b[bad] += (g.uniform(-30, 30, (len(bad), 2)) * scale).astype(np.float32)
    return int(frame_us), int(next_us), a, b


def frame_us(k, start_s=1.0):
    return int(round((start_s + k / FPS) * 1e6))


def plant_range(cam, sizes, delay_s, readout_ms, velocity, seed, outliers=0.0, start_s=1.0):
    return [plant_pair(cam, n, frame_us(k, start_s), frame_us(k + 1, start_s), delay_s, readout_ms, velocity, seed + 7 * k, outliers) for k, n in enumerate(sizes)]


def unit(v, length):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v) * length


def cfg_of(cam, cfg):
    """abi.SyncRsCfg of a statement camera and RS.Cfg"""
    c = abi.SyncRsCfg(video_width=cam.video[0], video_height=cam.video[1], flow_width=cam.flow[0], flow_height=cam.flow[1], rounds=cfg.rounds, refine=cfg.refine,
                      hypotheses=cfg.hypotheses, refits=cfg.refits, jacobi_sweeps=cfg.sweeps, frame_readout_time_ms=cfg.readout_ms, step_s=cfg.step_s,
                      loss_scale=cfg.loss_scale)
    for i, v in enumerate(cam.K.reshape(9)):
        c.camera_matrix[i] = v
    return c


def rows_of(results):
    """[abi.SyncResult] -> the statement's rows"""
    return [(r.found, r.n_coarse, r.coarse_value, r.coarse_cost, r.value, r.cost) for r in results]


class Clip:
    """One planted search: a range of `pairs` x `points`, the truth `delay_ms`, searched from `initial_ms` over `radius_ms`"""

    def __init__(self, name, delay_ms, initial_ms=0.0, radius_ms=30.0, speed=0.5, outliers=0.0, readout_ms=12.0, rate_hz=1000.0, pairs=8, points=60, seed=11):
        self.name, self.delay_ms, self.initial_ms, self.radius_ms, self.readout_ms, self.rate_hz = name, delay_ms, initial_ms, radius_ms, readout_ms, rate_hz
        self.cam = ES.Camera(EC.pinhole_clip(), FLOW)
        self.cfg = RS.Cfg(readout_ms=readout_ms)
        self.track = track(rate_hz)
        self.ranges = [plant_range(self.cam, [points] * pairs, delay_ms / 1000.0, readout_ms, unit((1.0, 0.4, 0.2), speed), seed, outliers)]
        self._found = {}

    def searched(self, readout_ms=None, conj=False):
        """the statement's search (computed once per setting, shared, never modified)"""
        key = (readout_ms, conj)
        if key not in self._found:
            cfg = self.cfg if readout_ms is None else RS.Cfg(readout_ms=readout_ms)
            self._found[key] = RS.search(self.cam, cfg, self.track[0], self.track[1], self.ranges, self.initial_ms / 1000.0, self.radius_ms / 1000.0, conj)
        return self._found[key]


CLIPS = {
    # the delay cases (a small translation, clean points, 12 ms readout, 1 kHz)
    "d+7.3": lambda: Clip("d+7.3", 7.3),
    "d-41": lambda: Clip("d-41", -41.0, initial_ms=-40.0),
    "d-edge": lambda: Clip("d-edge", 29.5),                                           # within 1 ms of the search edge (30 ms)
    "d-outside": lambda: Clip("d-outside", 45.0),                                     # outside the search: the acceptance rule must refuse it
    # the clip cases
    "rotation-only": lambda: Clip("rotation-only", 7.3, speed=0.0),
    "large-translation": lambda: Clip("large-translation", 7.3, speed=3.0),
    "outliers": lambda: Clip("outliers", 7.3, outliers=0.3),
    "outliers-large": lambda: Clip("outliers-large", -41.0, initial_ms=-40.0, speed=3.0, outliers=0.3),
    "global-shutter": lambda: Clip("global-shutter", 7.3, readout_ms=0.01),
    "readout-12-negative": lambda: Clip("readout-12-negative", 7.3, readout_ms=-12.0),
    "track-200hz": lambda: Clip("track-200hz", 7.3, rate_hz=200.0),
    "track-200hz-outliers": lambda: Clip("track-200hz-outliers", -41.0, initial_ms=-40.0, rate_hz=200.0, outliers=0.3),
}
INSIDE = [n for n in CLIPS if n != "d-outside"]
_CLIPS = {}


def clip(name):
    if name not in _CLIPS:
        _CLIPS[name] = CLIPS[name]()
    return _CLIPS[name]


class Case:
    """A call of the device tiers: ranges, a track, the search's settings — equality only, the points need not be a scene's"""

    def __init__(self, name, lens, shape, rate_hz=1000.0, readout_ms=12.0, outliers=0.3, seed=5, **cfg):
        self.name, self.shape = name, shape
        self.cam = ES.Camera(lens(), FLOW)
        self.cfg = RS.Cfg(readout_ms=readout_ms, **cfg)
        self.track = track(rate_hz)
        v = unit((1.0, 0.4, 0.2), 0.5)
        pin = ES.Camera(EC.pinhole_clip(), FLOW)                                      # planted through the pinhole, read through the case's lens
        if shape == "gpu":
            self.radius_s, self.initial_s = 0.030, 0.0
            self.ranges = [plant_range(pin, SIZES_GPU, 0.0073, readout_ms, v, seed, outliers),
                           [],
                           plant_range(pin, [40, 33], 0.0073, readout_ms, v, seed + 1, outliers, start_s=-0.02)
                           + plant_range(pin, [40], 0.0073, readout_ms, v, seed + 2, outliers, start_s=TRACK_SECONDS - 0.02)]
        else:
            self.radius_s, self.initial_s = 0.006, 0.002
            self.ranges = [plant_range(pin, [5, 66, 9], 0.0033, readout_ms, v, seed, outliers), plant_range(pin, [12, 1, 70], 0.0033, readout_ms, v, seed + 3, outliers)]
        self._stmt = None

    @property
    def statement(self):
        """(results, candidates, costs) of tests/_rssyncstmt.search: computed once, shared, never modified"""
        if self._stmt is None:
            self._stmt = RS.search(self.cam, self.cfg, self.track[0], self.track[1], self.ranges, self.initial_s, self.radius_s)
            for a in self._stmt[1:]:
                a.setflags(write=False)
        return self._stmt


SPECS = {
    "gpu-pinhole": lambda: Case("gpu-pinhole", EC.pinhole_clip, "gpu"),
    "gpu-fisheye-200hz": lambda: Case("gpu-fisheye-200hz", PC.tele_fisheye_clip, "gpu", rate_hz=200.0, readout_ms=-12.0),
    "gpu-sony-h3": lambda: Case("gpu-sony-h3", PC.tele_sony_clip, "gpu", readout_ms=0.01, hypotheses=3, refits=1, rounds=2, refine=0),
    "emu-pinhole": lambda: Case("emu-pinhole", EC.pinhole_clip, "emu"),
}
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = SPECS[name]()
    return _CASES[name]


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.view(np.uint64)


def assert_search_equal(got, want, what):
    """(results, candidates, costs) bit for bit"""
    for r, (g, w) in enumerate(zip(got[0], want[0])):
        assert tuple(g[:2]) == tuple(w[:2]) and (bits(np.array(g[2:])) == bits(np.array(w[2:]))).all(), "%s: range %d result %r != %r" % (what, r, g, w)
    assert len(got[0]) == len(want[0])
    for name, g, w in (("candidates", got[1], want[1]), ("costs", got[2], want[2])):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        same = bits(g) == bits(w)
        assert same.all(), "%s: %s differ from the statement at %s: %r != %r" % (what, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])
