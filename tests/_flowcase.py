"""TEST INFRASTRUCTURE: the synthetic scenes pyramidal Lucas-Kanade optical flow is tested on (statement, host-interpreted kernels, device alike).

The texture is analytic: a sum of plane waves of random direction and 6 .. 60 px wavelength (more amplitude at the long ones), evaluated in float64 at coordinates
mapped by the homography K R K^-1 of a planted camera rotation and quantised to u8 — so the true destination of every point is known without resampling.  Frame t
shows the texture point X at x_t = K R_t K^-1 X: a point p of frame a lies at q = K (R_b R_a^-1) K^-1 p in frame b, the convention of tests/_posecase.plant_f64.
One rectangle of the texture is held at a constant 128 (the minEig exit); the contrast returns over a smooth 8 px ramp outside it.

The focal length is 600 px: the estimator's inlier angle, 0.05 degrees, subtends 600 tan(0.05 deg) = 0.5236 px there, and a fifth of that is 0.1047 px — the
0.1 px cap of tests/test_flow_statement.py is below a fifth of what the pose stage tolerates.

Shapes, the smallest at which each mechanism exists: 200 x 168 at stride 208 (its level 3 would be 25 x 21, so L = 2: the cut) and 384 x 216 (L = 3, odd sides
48 x 27 at level 3).  3 frames, pairs (0, 1), (1, 2), (0, 2), 70 features a frame (more than a wave's lanes in the compaction and no multiple of 64): random
interior points, points within 3 px of each border, points in the flat rectangle, border points whose motion leaves the frame, a NaN, an infinity, a point
outside the frame, points on the last row and column.  The planted motions reach about 6 px at level 0 for the pair (0, 2): the pyramid is needed."""
import numpy as np

from gyroflow_amd import synthetic as S
import _flowstmt as FS
import _posecase as PC
import _posestmt as PS
import _zoomstmt as Z

FOCAL = 600.0
N_FEATURES = 70
PAIRS = [(0, 1), (1, 2), (0, 2)]
STEP_DEG = [(0.1, 0.2, -0.3), (-0.05, 0.3, -0.18)]          # (roll, pitch, yaw) of frame 1 against 0 and of frame 2 against 1: f * angle = 2 .. 4 px a step
FLAT_HALF = 30                                               # the flat rectangle: 60 x 60 px of the texture around its centre
FLAT_RAMP = 8.0                                              # px over which the contrast returns outside it


def camera(size):
    lens = S.gopro_style_lens(*size)
    lens["model"], lens["k"], lens["f"] = "opencv_standard", [0.0] * 12, (FOCAL, FOCAL)
    return PS.Camera(Z.Clip("flow-pinhole", lens=lens, size=size, out=size), size, num_iters=64)


class Case:
    def __init__(self, name, width, height, stride, seed):
        self.name, self.width, self.height, self.stride = name, width, height, stride
        self.cam = camera((width, height))
        g = np.random.default_rng(seed)
        n_waves = 40
        lam = 6.0 * 10.0 ** g.uniform(0.0, 1.0, n_waves)                                       # 6 .. 60 px
        ang, self._phase = g.uniform(0.0, 2.0 * np.pi, n_waves), g.uniform(0.0, 2.0 * np.pi, n_waves)
        self._kx, self._ky = 2.0 * np.pi / lam * np.cos(ang), 2.0 * np.pi / lam * np.sin(ang)
        amp = lam ** 0.5 * g.uniform(0.5, 1.0, n_waves)
        self._amp = amp * 45.0 / np.sqrt(0.5 * (amp ** 2).sum())                                # a standard deviation of 45 gray levels
        self.flat = (width * 0.5 - FLAT_HALF, height * 0.5 - FLAT_HALF, width * 0.5 + FLAT_HALF, height * 0.5 + FLAT_HALF)
        self.R = [np.eye(3)]
        for step in STEP_DEG:
            self.R.append(PC.rotation_f64(*step) @ self.R[-1])
        ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
        self.frames = np.full((3, height, stride), 255, dtype=np.uint8)                         # (the padding of a row is not the picture)
        for t in range(3):
            X = self.move(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1), np.linalg.inv(self.R[t]))
            self.frames[t, :, :width] = np.clip(np.rint(self.texture(X)), 0, 255).astype(np.uint8).reshape(height, width)
        self.features = [self._features(g, t) for t in range(3)]
        self.pairs = PAIRS
        self._stmt = self._grid = None

    def texture(self, X):
        v = 128.0 + (self._amp[None, :] * np.cos(X[:, :1] * self._kx[None, :] + X[:, 1:] * self._ky[None, :] + self._phase[None, :])).sum(axis=1)
        x0, y0, x1, y1 = self.flat
        # the contrast falls to zero over FLAT_RAMP px outside the rectangle (a smooth step: a hard edge would alias in the u8 samples, and its position with it)
        d = np.maximum(np.maximum(x0 - X[:, 0], X[:, 0] - x1), np.maximum(y0 - X[:, 1], X[:, 1] - y1))
        t = np.clip(d / FLAT_RAMP, 0.0, 1.0)
        return 128.0 + (v - 128.0) * (t * t * (3.0 - 2.0 * t))

    def move(self, p, R):
        """K R K^-1 p in float64, p [n][2]"""
        K = self.cam.K
        H = K @ R @ np.linalg.inv(K)
        q = np.concatenate([np.asarray(p, dtype=np.float64), np.ones((len(p), 1))], axis=1) @ H.T
        return q[:, :2] / q[:, 2:]

    def rotation(self, a, b):
        return self.R[b] @ np.linalg.inv(self.R[a])

    def destination(self, a, b, p):
        """where the points p of frame a lie in frame b (float64)"""
        return self.move(p, self.rotation(a, b))

    def in_flat(self, t, p, margin=0.0):
        """whether the points p of frame t show the flat rectangle (grown by `margin`)"""
        X = self.move(p, np.linalg.inv(self.R[t]))
        x0, y0, x1, y1 = self.flat
        return (X[:, 0] >= x0 - margin) & (X[:, 0] < x1 + margin) & (X[:, 1] >= y0 - margin) & (X[:, 1] < y1 + margin)

    def _features(self, g, t):
        w, h = self.width, self.height
        centre = self.move(np.array([[w * 0.5, h * 0.5]]), self.R[t])[0]                         # the flat rectangle's centre as frame t shows it
        special = [(1.5, h * 0.3), (2.75, h * 0.7), (w - 1.25, h * 0.4), (w - 2.5, h * 0.6), (w * 0.3, 0.5), (w * 0.6, 2.25), (w * 0.4, h - 1.5), (w * 0.7, h - 3.0),      # within 3 px of each border
                   (0.0, 0.0), (w - 1.0, h - 1.0), (w - 1.0, 37.25), (50.5, h - 1.0),                                            # corners, the last column and row
                   (centre[0], centre[1]), (centre[0] + 3.5, centre[1] - 2.25), (centre[0] - 4.0, centre[1] + 3.0), (centre[0] - 1.0, centre[1] - 3.75),      # flat
                   (np.nan, 20.0), (30.0, np.inf), (-0.5, 10.0), (float(w), 12.0), (15.0, float(h))]                             # not tracked
        rnd = np.stack([g.uniform(4.0, w - 4.0, N_FEATURES - len(special)), g.uniform(4.0, h - 4.0, N_FEATURES - len(special))], axis=1)
        pts = np.concatenate([rnd[:20], np.array(special), rnd[20:]]).astype(np.float32)
        assert pts.shape == (N_FEATURES, 2)
        return pts

    @property
    def statement(self):
        """tests/_flowstmt.flow_pyrlk on the caller's features: computed once, shared, never modified"""
        if self._stmt is None:
            self._stmt = FS.flow_pyrlk(self.frames[:, :, :self.width], self.pairs, self.features)
            for a in self._stmt.values():
                a.setflags(write=False)
        return self._stmt

    @property
    def grid_statement(self):
        if self._grid is None:
            self._grid = FS.flow_pyrlk(self.frames[:, :, :self.width], self.pairs, None)
            for a in self._grid.values():
                a.setflags(write=False)
        return self._grid


class ExitCase(Case):
    """The iteration's out-of-level exit, which the analytic scene never takes.  96 x 64 at stride 100 (L = 1).  Every frame is a ramp of 2 gray levels a pixel in x
    plus smooth noise of its own; frames 1, 2 and 3 have the ramp displaced by +40, -40 and +12 px, so that the brightness a template holds lies far outside the second
    frame (or, at 12 px, just outside for a border feature) and the updates walk the guess out of [-21, n) — through every side, because the noise is not the same
    in the two frames and the walk wanders in y.  An upper level that is left hands its guess down: 2 (g + 10) - 10 of a g outside [-21, n_1) is outside
    [-21, n_0), so level 0 is then left at once, with 0 updates — that IS the continuation.  tests/test_flow_statement.py asserts which exit each feature takes
    (tests/_flowstmt.track's trace); the interpreter and device tiers compare the case to the bit like the others."""

    def __init__(self, name):
        self.name, self.width, self.height, self.stride = name, 96, 64, 100
        self.cam = camera((self.width, self.height))
        ys, xs = np.mgrid[0:self.height, 0:self.width].astype(np.float64)
        self.frames = np.full((4, self.height, self.stride), 255, dtype=np.uint8)
        for t, (shift, seed) in enumerate([(0, 1), (40, 2), (-40, 3), (12, 5)]):
            n = np.random.default_rng(seed).uniform(-1.0, 1.0, (self.height + 8, self.width + 8))
            k = np.ones(5) / 5.0
            n = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 0, n)
            n = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 1, n)[4:4 + self.height, 4:4 + self.width] * 60.0
            self.frames[t, :, :self.width] = np.clip(np.rint(2.0 * (xs - shift) + 30.0 + n), 0, 255).astype(np.uint8)
        pts = [(x + 0.5, y) for x in range(2, 96, 6) for y in (8.5, 30.25, 55.0)] + [(79.5, 4.5), (79.5, 8.5), (10.5, 30.25), (1.5, 60.5)]
        self.features = [np.array(pts, dtype=np.float32)] + [np.array(pts[:5], dtype=np.float32)] * 3
        self.pairs = [(0, 1), (0, 2), (0, 3)]
        self._stmt = self._grid = None

    def traces(self):
        """[pair][feature] -> {level: how it ended} (tests/_flowstmt.track)"""
        w = self.width
        pyr = [FS.pyramid(f[:, :w]) for f in self.frames]
        out = []
        for a, b in self.pairs:
            rows = []
            for x, y in self.features[a]:
                tr = []
                FS.track(pyr[a], pyr[b], x, y, tr)
                rows.append(dict(tr))
            out.append(rows)
        return out


_CASES = {}
SPECS = {"cut-200x168": lambda: Case("cut-200x168", 200, 168, 208, 5), "odd-384x216": lambda: Case("odd-384x216", 384, 216, 384, 6)}      # the analytic scene
EXIT_SPECS = {"exits-96x64": lambda: ExitCase("exits-96x64")}
ALL_SPECS = dict(SPECS, **EXIT_SPECS)                                   # what the interpreter and device tiers compare to the bit


def case(name):
    if name not in _CASES:
        _CASES[name] = ALL_SPECS[name]()
    return _CASES[name]


def raw_slices(c, grid_nodes=None):
    """-> one slice of the raw outputs per pair of the case"""
    out, raw = [], 0
    for a, _ in c.pairs:
        n = len(c.features[a]) if grid_nodes is None else grid_nodes
        out.append(slice(raw, raw + n))
        raw += n
    return out


OUTPUTS = ("next", "status", "iters", "pair_first", "points_a", "points_b")
GRID_OUTPUTS = OUTPUTS + ("grid_points", "grid_counts")


def assert_equal_to_statement(got, want, what, names=OUTPUTS):
    """bit for bit (floats compared as their bit patterns; a not-tracked NaN feature is copied, so even its bits agree)"""
    for name in names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        view = {1: np.uint8, 4: np.uint32}[g.dtype.itemsize]
        same = g.view(view) == w.view(view)
        assert same.all(), "%s: %s differs from the statement at %s: %r != %r" % (what, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])
