"""TEST INFRASTRUCTURE: the frames Shi-Tomasi corner detection is tested on (statement, host-interpreted kernels, device alike), each the smallest shape at which
its mechanism exists:

cut-200x168     the three frames of tests/_flowcase "cut-200x168" at stride 208, padding 255 (not picture): the list is exhausted before the cap of 200, and some
                positive local maxima lie at or below the threshold and must not be picked
odd-384x216     the three frames of tests/_flowcase "odd-384x216": the cap of 200 is reached; both sides odd
checker-72x64   ((x // 8 + y // 8) % 2) * 200 + 20: every candidate has ONE score — pure tie order
rects-160x120   four rectangles on a background of 40, clean and with uniform +-2 noise of seed 7: the corners are exactly the 16 rectangle-corner pixels
noise-40x48     default_rng(3).integers(0, 256): several tiles with partial edges
3x3, 5x4        random u8: one interior pixel (two), every read reflected

The statement's result of a (case, parameters) is computed once (`statement`), shared by the tiers, and never modified."""
import numpy as np

import _cornerstmt as CS
import _flowcase as FC

RECTS = [(20, 15, 55, 45, 200), (80, 20, 140, 50, 120), (30, 70, 70, 105, 90), (95, 65, 150, 110, 230)]      # (x0, y0, x1, y1, value), x1 / y1 exclusive


def rect_corner_pixels():
    return sorted((x, y) for x0, y0, x1, y1, _ in RECTS for x in (x0, x1 - 1) for y in (y0, y1 - 1))


def _rects(noise):
    img = np.full((120, 160), 40, dtype=np.int32)
    for x0, y0, x1, y1, v in RECTS:
        img[y0:y1, x0:x1] = v
    if noise:
        img += np.random.default_rng(7).integers(-2, 3, img.shape)
    return img.astype(np.uint8)[None]


def _checker():
    ys, xs = np.mgrid[0:64, 0:72]
    return (((xs // 8 + ys // 8) % 2) * 200 + 20).astype(np.uint8)[None]


class Case:
    def __init__(self, name, frames, width):
        self.name, self.frames, self.width = name, np.ascontiguousarray(frames, dtype=np.uint8), width
        self.frames.setflags(write=False)
        self.height, self.stride = self.frames.shape[1], self.frames.shape[2]


SPECS = {
    "cut-200x168": lambda: Case("cut-200x168", FC.case("cut-200x168").frames, 200),
    "odd-384x216": lambda: Case("odd-384x216", FC.case("odd-384x216").frames, 384),
    "checker-72x64": lambda: Case("checker-72x64", _checker(), 72),
    "rects-160x120": lambda: Case("rects-160x120", _rects(False), 160),
    "rects-noise-160x120": lambda: Case("rects-noise-160x120", _rects(True), 160),
    "noise-40x48": lambda: Case("noise-40x48", np.random.default_rng(3).integers(0, 256, (1, 48, 40)), 40),
    "3x3": lambda: Case("3x3", np.random.default_rng(11).integers(0, 256, (2, 3, 3)), 3),
    "5x4": lambda: Case("5x4", np.random.default_rng(12).integers(0, 256, (2, 4, 5)), 5),
}
NAMES = sorted(SPECS)
REFERENCE = dict(max_corners=CS.MAX_CORNERS, quality=CS.QUALITY, min_distance=CS.MIN_DISTANCE)
# the parameter variants: the cap (an exact prefix), the distance (0: no suppression), the quality (0.25: the threshold ends the rounds early)
VARIANTS = [dict(REFERENCE)] + [dict(REFERENCE, max_corners=m) for m in (64, 8)] + [dict(REFERENCE, min_distance=d) for d in (2.5, 1.0, 0.0)] + [dict(REFERENCE, quality=0.25)] + \
           [dict(max_corners=64, quality=0.25, min_distance=2.5)]
VARIANT_IDS = ["m%d-q%g-d%g" % (v["max_corners"], v["quality"], v["min_distance"]) for v in VARIANTS]

_CASES, _STATEMENTS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = SPECS[name]()
    return _CASES[name]


def statement(name, max_corners=CS.MAX_CORNERS, quality=CS.QUALITY, min_distance=CS.MIN_DISTANCE):
    key = (name, max_corners, quality, min_distance)
    if key not in _STATEMENTS:
        c = case(name)
        s = CS.detect_clip(c.frames, c.width, max_corners, quality, min_distance)
        for a in s.values():
            a.setflags(write=False)
        _STATEMENTS[key] = s
    return _STATEMENTS[key]


_CHAINS = {}


def chain(name):
    """the CPU chain on one of tests/_flowcase's analytic scenes: the statement's corners of every frame -> tests/_flowstmt.flow_pyrlk over _flowcase.PAIRS ->
    (features per frame, the flow statement's outputs).  Computed once, shared, never modified."""
    if name not in _CHAINS:
        import _flowstmt as FS
        c, s = case(name), statement(name)
        feats = [s["corners"][f, :s["counts"][f]] for f in range(len(c.frames))]
        flow = FS.flow_pyrlk(c.frames[:, :, :c.width], FC.PAIRS, feats)
        for a in flow.values():
            a.setflags(write=False)
        _CHAINS[name] = (feats, flow)
    return _CHAINS[name]


def chain_pairs(name):
    """-> [(points_a, points_b)] per pair of _flowcase.PAIRS, what the pose stage takes"""
    s = chain(name)[1]
    first = s["pair_first"]
    return [(s["points_a"][first[p]:first[p + 1]], s["points_b"][first[p]:first[p + 1]]) for p in range(len(first) - 1)]


OUTPUTS = ("corners", "scores", "counts", "feat_first", "features")


def assert_equal_to_statement(got, want, what, names=OUTPUTS):
    """bit for bit (floats compared as their bit patterns)"""
    for name in names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), "%s: %s differs from the statement at %s: %r != %r" % (what, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])
