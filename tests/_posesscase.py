"""TEST INFRASTRUCTURE: the frame pairs the essential-matrix pose estimation is tested on (statement, host-interpreted kernels, device alike).

  plant_scene    the plant of tests/test_pose_essential_statement.py, an independent float64 path: a 3-D scene (x +-4, y +-2.5, z 3 .. 20) seen by a pinhole of
                 1920 x 1080 at f = 1000 before and after a rotation of up to 2 degrees an axis and a translation of length |t| in a random direction; pixels
                 rounded to f32; 30 % of the second frame's points displaced by up to +-40 px an axis.
  plant_frame    for the equality cases under real lenses, where all that matters is that rounds differ in their inliers and the refit runs: first-frame pixels
                 uniform inside the flow image at depths 3 .. 20 through the lens' f and c as a pinhole, the same motion, 10 % outliers (an octet is clean in
                 4 rounds of 10).  The lenses are the nearly-pinhole ones of tests/_posecase.py, so the clean points stay within the threshold.

CASES: pairs of 0, 7, 8, 9, 63, 64, 65 and 200 points; 1, 7, 64, 65 and 257 rounds (one more than the fit workgroup's 256 lanes); a flow image of half the video's
size; the fisheye; a generic lens (sony) under a digital stretch; a point without a lens inverse."""
import numpy as np

from gyroflow_amd import abi
from gyroflow_amd import synthetic as S
import _posecase as PC
import _posessstmt as ES
import _zoomstmt as Z

SIZES = [0, 7, 8, 9, 63, 64, 65, 200]
FIT_LANES = 256                                  # GFW_PE_LANES: a fit workgroup is 256 rounds of a pair


def pinhole_clip(size=(1920, 1080), f=1000.0):
    lens = S.gopro_style_lens(*size)
    lens["model"], lens["k"], lens["f"] = "opencv_standard", [0.0] * 12, (f, f)
    return Z.Clip("pinhole", lens=lens, size=size, out=size)


def rotation_vector(rv):
    """Rodrigues in float64"""
    th = np.linalg.norm(rv)
    if th == 0.0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _move(g, X, tnorm, K, scale, outliers):
    n = len(X)
    R = rotation_vector(np.radians(g.uniform(-2, 2, 3)))
    t = g.normal(size=3)
    t = t / np.linalg.norm(t) * tnorm
    X2 = X @ R.T + t
    c = np.array([K[0, 2], K[1, 2]])
    fxy = np.array([K[0, 0], K[1, 1]])
    p1 = ((X[:, :2] / X[:, 2:] * fxy + c) * scale).astype(np.float32)
    p2 = ((X2[:, :2] / X2[:, 2:] * fxy + c) * scale).astype(np.float32)
    bad = g.permutation(n)[:int(outliers * n)]
    p2[bad] += (g.uniform(-40, 40, (len(bad), 2)) * scale).astype(np.float32)
    clean = np.ones(n, dtype=bool)
    clean[bad] = False
    return p1, p2, R, clean


def plant_scene(cam, n, tnorm, seed, outliers=0.3):
    """-> (points_a, points_b f32 [n][2], R f64 [3][3], clean bool [n])"""
    g = np.random.default_rng(seed)
    X = np.stack([g.uniform(-4, 4, n), g.uniform(-2.5, 2.5, n), g.uniform(3, 20, n)], axis=1)
    return _move(g, X, tnorm, cam.K, np.array(cam.flow, dtype=np.float64) / np.array(cam.video, dtype=np.float64), outliers)


def plant_frame(cam, n, tnorm, seed, outliers=0.1):
    g = np.random.default_rng(seed)
    K = cam.K
    px = g.uniform(0.15, 0.85, (n, 2)) * np.array(cam.video, dtype=np.float64)
    z = g.uniform(3, 20, n)
    X = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], axis=1)
    a, b, _, _ = _move(g, X, tnorm, K, np.array(cam.flow, dtype=np.float64) / np.array(cam.video, dtype=np.float64), outliers)
    return a, b


def draws(counts, num_iters, seed, k=8):
    """numpy draws for the tiers that run without the library's generator: k distinct indices a round -> int32 [n_pairs][num_iters][k]"""
    g = np.random.default_rng(seed)
    out = np.zeros((len(counts), num_iters, k), dtype=np.int32)
    for p, n in enumerate(counts):
        if n >= k:
            for it in range(num_iters):
                out[p, it] = g.permutation(n)[:k]
    return out


def cfg_of(cam):
    c = abi.PoseEssentialCfg(video_width=cam.video[0], video_height=cam.video[1], flow_width=cam.flow[0], flow_height=cam.flow[1],
                             num_iters=cam.num_iters, inlier_threshold=cam.inlier_threshold, min_front=cam.min_front)
    for i, v in enumerate(cam.K.reshape(9)):
        c.camera_matrix[i] = v
    return c


class Case:
    def __init__(self, name, clip, sizes, num_iters, seed=3, flow=(320, 180), none_point=False, stretch=None, threshold=1e-6, min_front=10):
        self.name = name
        self.cam = ES.Camera(clip, flow, num_iters=num_iters, inlier_threshold=threshold, min_front=min_front)
        if stretch:
            self.cam.kp.input_horizontal_stretch, self.cam.kp.input_vertical_stretch = stretch
        self.pairs = [plant_frame(self.cam, n, 0.3, seed + 10 * i) for i, n in enumerate(sizes)]
        if none_point:                                   # the first pair's point 5 where the lens has no inverse
            self.pairs[0][0][5], self.pairs[0][1][5] = PC.NONE_A, PC.NONE_B
        self.octets = draws(sizes, num_iters, seed)
        self._stmt = None

    @property
    def statement(self):
        """(quats, rotations, essential, best, round_inliers, round_fits) of tests/_posessstmt.py: computed once, shared, never modified"""
        if self._stmt is None:
            self._stmt = ES.estimate(self.cam, self.pairs, self.octets)
            for a in self._stmt:
                a.setflags(write=False)
        return self._stmt


_CASES = {}
SPECS = {
    "fisheye-r7": lambda: Case("fisheye-r7", PC.tele_fisheye_clip(), SIZES, 7),
    "fisheye-r1": lambda: Case("fisheye-r1", PC.tele_fisheye_clip(), [8, 65], 1),
    "fisheye-r64": lambda: Case("fisheye-r64", PC.tele_fisheye_clip(), [12, 65], 64),
    "fisheye-r65": lambda: Case("fisheye-r65", PC.tele_fisheye_clip(), [65, 7, 9], 65),
    "fisheye-r257": lambda: Case("fisheye-r257", PC.tele_fisheye_clip(), [9, 65], FIT_LANES + 1),
    "fisheye-half-r7": lambda: Case("fisheye-half-r7", PC.tele_fisheye_clip(), [12, 65], 7, flow=(160, 90)),
    "cvstd-none-r7": lambda: Case("cvstd-none-r7", PC.none_lens_clip(), [12, 65], 7, none_point=True, min_front=5),
    "sony-stretch-r7": lambda: Case("sony-stretch-r7", PC.tele_sony_clip(), [0, 8, 64, 65, 200], 7, stretch=PC.STRETCH),
    "sony-stretch-r65": lambda: Case("sony-stretch-r65", PC.tele_sony_clip(), [65, 12], 65, stretch=PC.STRETCH),
}


def case(name):
    if name not in _CASES:
        _CASES[name] = SPECS[name]()
    return _CASES[name]


NAMES = ("quats", "rotations", "essential", "best", "round_inliers", "round_fits")


def assert_equal_to_statement(got, want, what, names=NAMES):
    """bit for bit (floats compared as their bit patterns; a NaN is a NaN: hosts and the device differ in the sign they give a generated one)"""
    for name, g, w in zip(names, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        view = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        same = g.view(view) == w.view(view)
        if g.dtype.kind == "f":
            same |= np.isnan(g) & np.isnan(w)
        assert same.all(), "%s: %s differs from the statement at %s: %r != %r" % (what, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])
