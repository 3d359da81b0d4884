"""TEST INFRASTRUCTURE: the frame pairs Almeida pose estimation is tested on (statement, host-interpreted kernels, device alike).

Two ways of planting a rotation into a pair's flow:
  plant_f64      an independent float64 path for tests/test_pose_statement.py: the f64 ray of `a` rotated, projected, rounded to f32 pixels.  The lens is a pinhole
                 (opencv_standard, zero coefficients): the reference's estimator compares a flow measured in source pixels with `delta`, which ends in undistorted
                 pixels (almeida.rs:58-68), so it recovers a rotation exactly only where the two agree.
  plant_f32      through the statement's own `delta` for the equality cases under real lenses, where all that matters is that rounds differ in their inliers.

CASES: what the interpreted kernels and the device run — pairs of 0, 1, 2, 3, 12, 63, 64, 65 and 200 points; 1, 7, 64 and 65 rounds; num_samples 40 against 65 points
with explicit lists; the fisheye and a generic lens (sony) under a digital lens (stretch); a point without a lens inverse."""
import numpy as np

from gyroflow_amd import abi
from gyroflow_amd import synthetic as S
import _posestmt as PS
import _zoomstmt as Z

SIZES = [0, 1, 2, 3, 12, 63, 64, 65, 200]


def pinhole_clip(size=(1920, 1080)):
    lens = S.gopro_style_lens(*size)
    lens["model"], lens["k"] = "opencv_standard", [0.0] * 12
    return Z.Clip("pinhole", lens=lens, size=size, out=size)


def rotation_f64(roll_deg, pitch_deg, yaw_deg):
    r, p, y = np.radians([roll_deg, pitch_deg, yaw_deg])
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return rz @ ry @ rx


def _outliers(g, n, fraction):
    """-> (is_outlier [n], gross flow [n][2] in normalised units: 0.01 .. 0.05 long, any direction)"""
    bad = np.zeros(n, dtype=bool)
    bad[g.permutation(n)[:int(round(fraction * n))]] = True
    length, angle = g.uniform(0.01, 0.05, n), g.uniform(0.0, 2.0 * np.pi, n)
    return bad, np.stack([length * np.cos(angle), length * np.sin(angle)], axis=1) * bad[:, None]


def plant_f64(cam, n, angles_deg, outlier_fraction, seed):
    """-> (points_a, points_b f32 [n][2], R f64 [3][3], clean bool [n]) on a pinhole camera"""
    g = np.random.default_rng(seed)
    flow, video = np.array(cam.flow, dtype=np.float64), np.array(cam.video, dtype=np.float64)
    a = (g.uniform(0.1, 0.9, (n, 2)) * flow).astype(np.float32)
    R = rotation_f64(*angles_deg)
    px = a.astype(np.float64) / flow * video
    K = cam.K
    ray = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1], np.ones(n)], axis=1)
    p3 = ray @ R.T
    moved = np.stack([K[0, 0] * p3[:, 0] / p3[:, 2] + K[0, 2], K[1, 1] * p3[:, 1] / p3[:, 2] + K[1, 2]], axis=1)
    bad, gross = _outliers(g, n, outlier_fraction)
    b = ((moved / video + gross) * flow).astype(np.float32)
    return a, b, R, ~bad


def plant_f32(cam, n, q, outlier_fraction, seed):
    """-> (points_a, points_b f32 [n][2]): the flow is the statement's delta under q, plus gross outliers"""
    g = np.random.default_rng(seed)
    flow = np.array(cam.flow, dtype=np.float32)
    a = (g.uniform(0.15, 0.85, (n, 2)) * flow).astype(np.float32)
    if n == 0:
        return a, a.copy()
    P = PS.prepare(cam, a, a)
    d = PS.delta(cam, PS.kr(cam.K, PS.qmatrix(np.asarray(q, dtype=np.float32)[None])), P["ray"][None], P["pos"][None])[0]
    _, gross = _outliers(g, n, outlier_fraction)
    return a, (a + (d + gross.astype(np.float32)) * flow).astype(np.float32)


def cfg_of(cam):
    c = abi.PoseAlmeidaCfg(video_width=cam.video[0], video_height=cam.video[1], flow_width=cam.flow[0], flow_height=cam.flow[1],
                           num_iters=cam.num_iters, num_samples=cam.num_samples, inlier_angle_deg=float(cam.inlier_angle))
    for i, v in enumerate(cam.K.reshape(9)):
        c.camera_matrix[i] = v
    return c


def draws(counts, num_iters, num_samples, seed, lists):
    """numpy draws for the tiers that run without the library's generator: distinct triples, permutation prefixes"""
    g = np.random.default_rng(seed)
    triples = np.zeros((len(counts), num_iters, 3), dtype=np.int32)
    samples = []
    for p, n in enumerate(counts):
        m = min(n, num_samples)
        if n >= 3:
            for it in range(num_iters):
                triples[p, it] = g.permutation(n)[:3]
        samples.append(np.array([g.permutation(n)[:m] for _ in range(num_iters)], dtype=np.int32).reshape(num_iters, m))
    return triples, (samples if lists else None)


# The estimator's three "derivative" vectors are whole deltas under a 0.001 degree rotation (almeida.rs:69-77), and a delta ends in UNDISTORTED pixels while it
# starts from source pixels (:65-67): under a lens that distorts by more than such a rotation moves a point (f / w * 1.7e-5 of the width) the vectors are the
# distortion itself, the 3 x 3 system is close to singular and no round has inliers.  That is the reference's behaviour and one case below keeps it ("gopro-style");
# the others run the fisheye and the sony bodies with coefficients that make them nearly a pinhole (theta_d = tan theta as far as the model's terms reach, at a long
# focal length), so that rounds have inliers and the refit runs: what is compared is bits, but bits of every path.
def tele_fisheye_clip():
    lens = S.gopro_style_lens(320, 180)
    lens["f"], lens["k"] = (640.0, 640.0), [1.0 / 3.0, 2.0 / 15.0, 17.0 / 315.0, 62.0 / 2835.0] + [0.0] * 8      # tan t = t (1 + t^2/3 + 2 t^4/15 + 17 t^6/315 + 62 t^8/2835 + ..)
    return Z.Clip("tele-fisheye", lens=lens)


def tele_sony_clip():
    """the sony polynomial as tan theta to the fifth power at f = 3 w, under the digital stretch (1.1, 0.95) that the input stretches of `STRETCH` undo"""
    lens = S.gopro_style_lens(320, 180)
    lens["model"], lens["f"], lens["k"] = "sony", (960.0, 960.0), [1.0, 0.0, 1.0 / 3.0, 0.0, 2.0 / 15.0, 0.0] + [0.0] * 6
    return Z.Clip("tele-sony-stretch", lens=lens, digital="digital_stretch", digital_params=[1.1, 0.95], seed=13)


STRETCH = (1.1, 0.95)


def none_lens_clip():
    """opencv_standard with k1 = -1e-5 at f = 3 w: nearly a pinhole inside the frame, no inverse where 1 + k1 r^2 < 0 (cvstd undistort_point: icdist < 0 -> None), r > 316"""
    lens = S.gopro_style_lens(320, 180)
    lens["model"], lens["f"], lens["k"] = "opencv_standard", (960.0, 960.0), [-1e-5] + [0.0] * 11
    return Z.Clip("cvstd-none", lens=lens)


NONE_A, NONE_B = (192080.0, 45.0), (192081.0, 45.0)      # flow pixels: 400 focal lengths right of the principal point


def none_case(num_iters=8):
    """-> (camera, points_a, points_b, planted q): 12 clean points, point 5 moved to where the lens has no inverse"""
    cam = PS.Camera(none_lens_clip(), (160, 90), num_iters=num_iters)
    q = PS.euler_quat(*[np.array([np.radians(v)], dtype=np.float32) for v in (1.0, 0.5, -1.0)])[0]
    a, b = plant_f32(cam, 12, q, 0.0, 21)
    a[5], b[5] = NONE_A, NONE_B
    return cam, a, b, q


class Case:
    def __init__(self, name, clip, sizes, num_iters, num_samples=1000, lists=False, seed=3, flow=(160, 90), none_point=False, stretch=None):
        self.name = name
        self.cam = PS.Camera(clip, flow, num_iters=num_iters, num_samples=num_samples)
        if stretch:
            self.cam.kp.input_horizontal_stretch, self.cam.kp.input_vertical_stretch = stretch
        q = PS.euler_quat(*[np.array([np.radians(v)], dtype=np.float32) for v in (1.5, -2.0, 0.8)])[0]
        self.pairs = [plant_f32(self.cam, n, q, 0.25, seed + 10 * i) for i, n in enumerate(sizes)]
        if none_point:                                   # the first pair's point 5 where the lens has no inverse
            self.pairs[0][0][5], self.pairs[0][1][5] = NONE_A, NONE_B
        self.triples, self.samples = draws(sizes, num_iters, num_samples, seed, lists)
        self._stmt = None

    @property
    def statement(self):
        """(quats, rotations, best, round_inliers, round_fits) of tests/_posestmt.py: computed once, shared, never modified"""
        if self._stmt is None:
            self._stmt = PS.estimate(self.cam, self.pairs, self.triples, self.samples)
            for a in self._stmt:
                a.setflags(write=False)
        return self._stmt


_CASES = {}
SPECS = {
    "fisheye-r7": lambda: Case("fisheye-r7", tele_fisheye_clip(), SIZES, 7),
    "fisheye-r1": lambda: Case("fisheye-r1", tele_fisheye_clip(), [3, 12], 1),
    "fisheye-r64-lists": lambda: Case("fisheye-r64-lists", tele_fisheye_clip(), [12, 65], 64, num_samples=40, lists=True),
    "fisheye-r65-lists": lambda: Case("fisheye-r65-lists", tele_fisheye_clip(), [65, 3], 65, num_samples=40, lists=True),
    "gopro-style-r7": lambda: Case("gopro-style-r7", Z.Clip("fisheye"), [12, 65], 7),
    "cvstd-none-r7": lambda: Case("cvstd-none-r7", none_lens_clip(), [12, 65], 7, none_point=True),
    "sony-stretch-r7": lambda: Case("sony-stretch-r7", tele_sony_clip(), [0, 3, 64, 65, 200], 7, stretch=STRETCH),
    "sony-stretch-r65-lists": lambda: Case("sony-stretch-r65-lists", tele_sony_clip(), [65, 12], 65, num_samples=40, lists=True, stretch=STRETCH),
}


def case(name):
    if name not in _CASES:
        _CASES[name] = SPECS[name]()
    return _CASES[name]


def assert_equal_to_statement(got, want, what):
    """quaternions, rotations, best, round_inliers, round_fits: bit for bit (floats compared as their bit patterns)"""
    names = ("quats", "rotations", "best", "round_inliers", "round_fits")
    for name, g, w in zip(names, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        view = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        same = g.view(view) == w.view(view)
        if g.dtype.kind == "f":
            same |= np.isnan(g) & np.isnan(w)                # (a NaN is a NaN: hosts and the device differ in the sign they give a generated one)
        assert same.all(), "%s: %s differs from the statement at %s: %r != %r" % (what, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])
