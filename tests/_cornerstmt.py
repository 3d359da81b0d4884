"""TEST INFRASTRUCTURE: the statement gfw_corners_shi_tomasi is held to — what `OFOpenCVPyrLK::detect_features` (optical_flow/opencv_pyrlk.rs:25-42) asks of
good_features_to_track(img, 200, 0.01, 10.0, no mask, blockSize 3, useHarris false, 0.04).  OpenCV's source is not part of the reference tree and OpenCV is not a
dependency: this is the published Shi-Tomasi / goodFeaturesToTrack scheme with the reference's parameters, operation by operation (builder-written;
tests/test_corner_statement.py holds it to its purpose first).

For one u8 frame w x h:
1. Dx, Dy: the 3 x 3 Sobel of the image as int32 on reflect-101 indices (-1 -> 1, n -> n - 2); |D| <= 1020.
2. Sxx, Sxy, Syy: the 3 x 3 unnormalised box sums of Dx^2, Dx Dy, Dy^2.  The box filter reflects the PRODUCT MAPS (reflect-101), as OpenCV filters `cov` — NOT the
   Sobel of a reflected image (the two differ in the sign of Dx Dy on the border).  Each sum is below 9 * 1020^2 < 2^24: exact in int32 and in its f32 conversion.
3. In f32, one rounding per operation: a = Sxx * 0.5, c = Syy * 0.5, b = Sxy, e = (a + c) - sqrt((a - c)^2 + b^2), sqrt correctly rounded.  OpenCV's scale
   1 / (12 * 255) is DROPPED: the selection depends only on e relative to the frame's maximum, and a common power-free factor would add a rounding; the scores are
   the unscaled e.  e can round slightly below 0.
4. t = max(max over ALL pixels of e, 0) * quality, one f32 product; k = e if e > t else 0.
5. Candidates: interior pixels (1 <= x <= w - 2, 1 <= y <= h - 2) with k != 0 and k == the 3 x 3 maximum of k; plateaus count in full.  Equivalent
   (`candidates_raw`): e > t and e >= all eight neighbours' e.
6. Order: by the unique 64-bit key bits(e) << 32 | (y w + x), descending (on a tie the larger pixel index first, like OpenCV's pointer tie-break).
7. Pick: walk the candidates in that order, accept one unless an accepted one lies closer than min_distance: (float)(dx^2 + dy^2) < min_distance * min_distance
   (one int -> f32 conversion, one f32 product); min_distance < 1 accepts everything; stop at max_corners.  A corner is (float x, float y) in pick order.
Equivalent form of the walk (`pick_rounds`, what the device runs; no sort): repeat <= max_corners times — take the largest key still alive, stop if its e <= t,
accept it, kill every alive candidate closer than min_distance, itself included."""
import numpy as np

MAX_CORNERS, QUALITY, MIN_DISTANCE = 200, 0.01, 10.0                   # opencv_pyrlk.rs:32-33


def reflect(i, n):
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * n - 2 - i, i)


def _shifted(m, dy, dx):
    """m at (reflect(y + dy), reflect(x + dx))"""
    h, w = m.shape
    return m[reflect(np.arange(h) + dy, h)][:, reflect(np.arange(w) + dx, w)]


def derivatives(img):
    p = np.asarray(img).astype(np.int32)
    s = lambda dy, dx: _shifted(p, dy, dx)
    dx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    dy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return dx, dy


def box_sums(img):
    """-> Sxx, Sxy, Syy int64 (asserted below 2^24 by the tests)"""
    dx, dy = derivatives(img)
    out = []
    for m in (dx * dx, dx * dy, dy * dy):
        m = m.astype(np.int64)
        out.append(sum(_shifted(m, j, i) for j in (-1, 0, 1) for i in (-1, 0, 1)))
    return out


def min_eigen(img):
    """-> e f32 [h][w], one rounding per operation"""
    sxx, sxy, syy = box_sums(img)
    f = np.float32
    a, c, b = sxx.astype(f) * f(0.5), syy.astype(f) * f(0.5), sxy.astype(f)
    d = a - c
    return ((a + c) - np.sqrt((d * d) + (b * b))).astype(f)


def threshold(e, quality):
    return np.float32(max(np.float32(e.max()), np.float32(0.0))) * np.float32(quality)


def _interior(mask):
    m = np.zeros_like(mask)
    m[1:-1, 1:-1] = mask[1:-1, 1:-1]
    return m


def candidates(e, t):
    """the statement's form -> bool [h][w]"""
    k = np.where(e > t, e, np.float32(0.0))
    pad = np.pad(k, 1, mode="constant", constant_values=-np.inf)          # (only interior pixels are asked: the pad is never the deciding value)
    h, w = k.shape
    mx = np.max([pad[1 + j:1 + j + h, 1 + i:1 + i + w] for j in (-1, 0, 1) for i in (-1, 0, 1)], axis=0)
    return _interior((k != 0) & (k == mx))


def candidates_raw(e, t):
    """the equivalent form on raw e: e > t and e >= all eight neighbours"""
    pad = np.pad(e, 1, mode="constant", constant_values=-np.inf)
    h, w = e.shape
    ok = e > t
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            if i or j:
                ok &= e >= pad[1 + j:1 + j + h, 1 + i:1 + i + w]
    return _interior(ok)


def keys(e, mask):
    """the 64-bit keys of the masked pixels (unsorted, row-major)"""
    ys, xs = np.nonzero(mask)
    w = e.shape[1]
    bits = e[ys, xs].view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (ys * w + xs).astype(np.uint64)


def _near(x, y, ax, ay, min_distance):
    d = (np.asarray(ax, dtype=np.int64) - x) ** 2 + (np.asarray(ay, dtype=np.int64) - y) ** 2
    return d.astype(np.float32) < np.float32(min_distance) * np.float32(min_distance)


def pick_sorted(key, w, max_corners, min_distance):
    """the sorted walk -> the accepted keys in pick order"""
    out, ax, ay = [], [], []
    for k in np.sort(key)[::-1]:
        if len(out) >= max_corners:
            break
        idx = int(k & np.uint64(0xFFFFFFFF))
        x, y = idx % w, idx // w
        if min_distance >= 1 and len(out) and _near(x, y, ax, ay, min_distance).any():
            continue
        out.append(k); ax.append(x); ay.append(y)
    return np.array(out, dtype=np.uint64)


def pick_rounds(key, w, max_corners, min_distance, t=None, stats=None):
    """the arg-max rounds; `key` may hold candidates at or below the threshold (every positive local maximum, as the device lists them): a round whose best e <= t
    ends the pick.  stats: dict that receives the rounds taken."""
    alive = np.array(key, dtype=np.uint64)
    idx = (alive & np.uint64(0xFFFFFFFF)).astype(np.int64)
    xs, ys = idx % w, idx // w
    live = np.ones(len(alive), dtype=bool)
    out = []
    rounds = 0
    while len(out) < max_corners and live.any():
        rounds += 1
        i = int(np.argmax(np.where(live, alive, np.uint64(0))))
        if t is not None and not (np.uint32(alive[i] >> np.uint64(32)).view(np.float32) > t):
            break
        out.append(alive[i])
        kill = _near(xs[i], ys[i], xs, ys, min_distance)
        kill[i] = True
        live &= ~kill
    if stats is not None:
        stats["rounds"] = rounds
    return np.array(out, dtype=np.uint64)


def detect(img, max_corners=MAX_CORNERS, quality=QUALITY, min_distance=MIN_DISTANCE, stats=None):
    """-> (corners f32 [k][2] in pick order, scores f32 [k])"""
    img = np.asarray(img)
    e = min_eigen(img)
    t = threshold(e, quality)
    key = keys(e, candidates(e, t))
    if stats is not None:
        stats["candidates"], stats["threshold"] = len(key), t
    got = pick_sorted(key, img.shape[1], max_corners, min_distance)
    idx = (got & np.uint64(0xFFFFFFFF)).astype(np.int64)
    w = img.shape[1]
    corners = np.stack([idx % w, idx // w], axis=1).astype(np.float32).reshape(-1, 2)
    return corners, (got >> np.uint64(32)).astype(np.uint32).view(np.float32)


def detect_clip(frames, width, max_corners=MAX_CORNERS, quality=QUALITY, min_distance=MIN_DISTANCE):
    """every output of gfw_corners_shi_tomasi for frames u8 [n][h][stride] -> dict(corners [n][max][2], scores [n][max], counts [n], feat_first [n + 1],
    features [total][2])"""
    n = len(frames)
    o = {"corners": np.zeros((n, max_corners, 2), dtype=np.float32), "scores": np.zeros((n, max_corners), dtype=np.float32), "counts": np.zeros(n, dtype=np.int32),
         "feat_first": np.zeros(n + 1, dtype=np.int32)}
    for f in range(n):
        c, s = detect(frames[f][:, :width], max_corners, quality, min_distance)
        o["corners"][f, :len(c)], o["scores"][f, :len(c)], o["counts"][f] = c, s, len(c)
    o["feat_first"][1:] = np.cumsum(o["counts"])
    o["features"] = np.concatenate([o["corners"][f, :o["counts"][f]] for f in range(n)]).reshape(-1, 2) if n else np.zeros((0, 2), dtype=np.float32)
    return o
