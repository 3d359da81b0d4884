"""TEST INFRASTRUCTURE: the statement gfw_flow_pyrlk is held to — pyramidal Lucas-Kanade optical flow as `OFOpenCVPyrLK::optical_flow_to`
(src/core/synchronization/optical_flow/opencv_pyrlk.rs:63-119) asks it of calcOpticalFlowPyrLK: window 21 x 21, maxLevel 3, 30 iterations or eps 0.01, flags 0,
minEigThreshold 1e-4 — numpy, operation by operation.  OpenCV's source is not part of the reference tree and OpenCV is not a dependency: this is a builder-written
statement after the published scheme (Bouguet, "Pyramidal implementation of the Lucas Kanade feature tracker"), held to its purpose by tests/test_flow_statement.py
before anything is compared with it.

Every window sum is an INTEGER, so a parallel reduction may take any order and still equal this to the bit:
  frames    n u8 gray planes of one width x height.
  pyramid   level l + 1 has sides (w_l + 1) / 2, (h_l + 1) / 2; out(x, y) = (sum_{i,j=-2..2} k_i k_j in(r(2x + i), r(2y + j)) + 128) >> 8, k = 1 4 6 4 1, r reflect-101
            (-1 -> 1, n -> n - 2).  Levels 0 .. L, L the largest l <= 3 whose two sides are both >= 24: the window then reflects at most once (gfw_flow.hip's proof).
  Scharr    Dx(x, y) = 3 (A(x+1, y-1) - A(x-1, y-1)) + 10 (A(x+1, y) - A(x-1, y)) + 3 (A(x+1, y+1) - A(x-1, y+1)) on reflected indices, Dy its transpose; |D| <= 4080.
  feature (px, py) of frame A into frame B, levels l = L .. 0:
    1. u = (px, py) * 2^-l - 10 (f32).  g = u at level L, below it g = 2 * r - 10 with r = g + 10 the level above's result (each one f32 operation).
    2. weights of a fraction (a, b): w00 = rint(((1-a)(1-b)) 16384), w01 = rint((a (1-b)) 16384), w10 = rint(((1-a) b) 16384), w11 = 16384 - w00 - w01 - w10.
    3. template at iu = floor(u), u's weights, 21 x 21: I = (sum w A_l + 256) >> 9, Ix = (sum w Dx + 8192) >> 14, Iy alike (arithmetic shifts);
       A11 = sum Ix^2, A12 = sum Ix Iy, A22 = sum Iy^2 in int64.
    4. f32, s = 2^-20: a11 = f32(A11) s ..; D = a11 a22 - a12 a12; minEig = ((a22 + a11) - sqrt((a11 - a22)(a11 - a22) + 4 a12 a12)) / 882; the level is skipped when
       minEig < 1e-4 or D < FLT_EPSILON (the guess passes down; at level 0 status 0); else D = 1 / D.
    5. j = 0 .. 29: the level ends when g is not finite or |g| >= 2^24 (tested before any cast), or iv = floor(g) has iv.x < -21, iv.x >= w_l, iv.y < -21, iv.y >= h_l
       (either at level 0: status 0).  J from B_l at iv with g's weights as I; B1 = sum (J - I) Ix, B2 = sum (J - I) Iy (int64); b = f32(B) s;
       dx = (a12 b2 - a22 b1) D, dy = (a12 b1 - a11 b2) D; g += d; stop when dx dx + dy dy <= 1e-4; stop when j > 0 and |dx + pdx| < 0.01 and |dy + pdy| < 0.01,
       after g -= 0.5 d; pd = d.  iters[l] = the updates made (-1 for a level not built or skipped).
    6. next = g + 10, status 1 unless cleared.  A feature that is not finite or outside [0, w) x [0, h) is not tracked: status 0, next = the feature.
  filter    (opencv_pyrlk.rs:88-100) kept: status 1 and both points in [0, w) x [0, h) as f32, in feature order.
  grid      (opencv_dis.rs:62-119) step = w / 15, win = max(10, round(w 0.02)), half = win / 2; for i in (0..w).step_by(step), for j in (0..h).step_by(step): the
            clipped window's sum, sum_sq, count as sequential f32 folds (ny outer, nx inner), variance = sum_sq / count - mean mean; the node is a feature when
            variance > 3.0."""
import numpy as np

f32 = np.float32
WIN, HALF, MAX_LEVEL, ITERS, SIDE_MIN = 21, 10, 3, 30, 24
FLT_EPSILON = f32(1.1920928955078125e-7)
_K = (1, 4, 6, 4, 1)


def reflect(i, n):
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * n - 2 - i, i)


def level_sizes(width, height):
    """-> [(w_l, h_l)] of the levels that are built"""
    out = [(width, height)]
    while len(out) <= MAX_LEVEL:
        w, h = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if w < SIDE_MIN or h < SIDE_MIN:
            break
        out.append((w, h))
    return out


def down(img):
    h, w = img.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    a = img.astype(np.int64)
    xs = reflect(2 * np.arange(dw)[None, :] + np.arange(-2, 3)[:, None], w)
    ys = reflect(2 * np.arange(dh)[None, :] + np.arange(-2, 3)[:, None], h)
    rows = sum(_K[i] * a[:, xs[i]] for i in range(5))
    out = sum(_K[j] * rows[ys[j], :] for j in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def pyramid(frame):
    """frame u8 [h][w] -> its levels"""
    levels = [np.ascontiguousarray(frame, dtype=np.uint8)]
    for _ in level_sizes(frame.shape[1], frame.shape[0])[1:]:
        levels.append(down(levels[-1]))
    return levels


def weights(a, b):
    na, nb = f32(1) - a, f32(1) - b
    w00 = int(np.rint((na * nb) * f32(16384)))
    w01 = int(np.rint((a * nb) * f32(16384)))
    w10 = int(np.rint((na * b) * f32(16384)))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def bilinear(X, W):
    """X int64 [22][22] at the window's 22 x 22 integer positions -> the weighted sums at its 21 x 21 pixels"""
    return W[0] * X[:-1, :-1] + W[1] * X[:-1, 1:] + W[2] * X[1:, :-1] + W[3] * X[1:, 1:]


_R24, _R22 = np.arange(24), np.arange(22)


def template(A, iux, iuy, W):
    lh, lw = A.shape
    P = A[reflect(iuy - 1 + _R24, lh)[:, None], reflect(iux - 1 + _R24, lw)[None, :]].astype(np.int64)       # rows / columns iu - 1 .. iu + 22
    dx = 3 * (P[:-2, 2:] - P[:-2, :-2]) + 10 * (P[1:-1, 2:] - P[1:-1, :-2]) + 3 * (P[2:, 2:] - P[2:, :-2])  # at positions iu .. iu + 21
    dy = 3 * (P[2:, :-2] - P[:-2, :-2]) + 10 * (P[2:, 1:-1] - P[:-2, 1:-1]) + 3 * (P[2:, 2:] - P[:-2, 2:])
    return (bilinear(P[1:-1, 1:-1], W) + 256) >> 9, (bilinear(dx, W) + 8192) >> 14, (bilinear(dy, W) + 8192) >> 14


def sample(B, ivx, ivy, W):
    lh, lw = B.shape
    P = B[reflect(ivy + _R22, lh)[:, None], reflect(ivx + _R22, lw)[None, :]].astype(np.int64)
    return (bilinear(P, W) + 256) >> 9


def track(pa, pb, px, py, trace=None):
    """One feature of frame A (pyramid pa) into frame B (pb) -> ((next x, next y) f32, status, iters [4]).  ``trace``: a list that receives (level, how the level
    ended): "skipped" (minEig / D), "guard" (g not finite or >= 2^24), "left" (floor(g) outside [-21, n)), "converged", "oscillated", "exhausted" — for the tests that
    have to know WHICH exit a case takes; no output depends on it."""
    px, py = f32(px), f32(py)
    h, w = pa[0].shape
    iters = [-1, -1, -1, -1]
    if not (px >= f32(0) and px < f32(w) and py >= f32(0) and py < f32(h)):
        return (px, py), 0, iters
    status, top = 1, len(pa) - 1
    s, ten, two = f32(2.0 ** -20), f32(10), f32(2)
    gx = gy = f32(0)
    for l in range(top, -1, -1):
        A, B = pa[l], pb[l]
        lh, lw = A.shape
        scale = f32(2.0 ** -l)
        ux, uy = (px * scale) - ten, (py * scale) - ten
        if l == top:
            gx, gy = ux, uy
        else:
            gx, gy = (two * (gx + ten)) - ten, (two * (gy + ten)) - ten
        fux, fuy = np.floor(ux), np.floor(uy)
        I, Ix, Iy = template(A, int(fux), int(fuy), weights(ux - fux, uy - fuy))
        a11, a12, a22 = f32(int((Ix * Ix).sum())) * s, f32(int((Ix * Iy).sum())) * s, f32(int((Iy * Iy).sum())) * s
        D = (a11 * a22) - (a12 * a12)
        dif = a11 - a22
        min_eig = ((a22 + a11) - np.sqrt((dif * dif) + ((f32(4) * a12) * a12))) / f32(882)
        if min_eig < f32(1e-4) or D < FLT_EPSILON:
            if l == 0:
                status = 0
            if trace is not None:
                trace.append((l, "skipped"))
            continue
        D = f32(1) / D
        pdx = pdy = f32(0)
        count, how = 0, "exhausted"
        for j in range(ITERS):
            if not (abs(gx) < f32(16777216)) or not (abs(gy) < f32(16777216)):
                if l == 0:
                    status = 0
                how = "guard"
                break
            fgx, fgy = np.floor(gx), np.floor(gy)
            if fgx < -21 or fgx >= lw or fgy < -21 or fgy >= lh:
                if l == 0:
                    status = 0
                how = "left"
                break
            d = sample(B, int(fgx), int(fgy), weights(gx - fgx, gy - fgy)) - I
            b1, b2 = f32(int((d * Ix).sum())) * s, f32(int((d * Iy).sum())) * s
            dx, dy = ((a12 * b2) - (a22 * b1)) * D, ((a12 * b1) - (a11 * b2)) * D
            gx, gy = gx + dx, gy + dy
            count = j + 1
            if ((dx * dx) + (dy * dy)) <= f32(1e-4):
                how = "converged"
                break
            if j > 0 and abs(dx + pdx) < f32(0.01) and abs(dy + pdy) < f32(0.01):
                gx, gy = gx - (f32(0.5) * dx), gy - (f32(0.5) * dy)
                how = "oscillated"
                break
            pdx, pdy = dx, dy
        iters[l] = count
        if trace is not None:
            trace.append((l, how))
    return (gx + ten, gy + ten), status, iters


def grid_dims(width, height):
    """-> (step, half, columns, rows): `i` runs over the columns (outer), `j` over the rows"""
    step = width // 15
    win = max(10, int(np.floor(np.float64(f32(width) * f32(0.02)) + 0.5)))   # f32::round of a positive value: the f32 product, then half away from zero (exact in f64)
    return step, win // 2, (width + step - 1) // step, (height + step - 1) // step


def grid_points(frame):
    """opencv_dis.rs:62-119 on one frame u8 [h][w] -> the kept nodes f32 [n][2] (i, j) in the loop's order"""
    h, w = frame.shape
    step, half, _, _ = grid_dims(w, h)
    out = []
    for i in range(0, w, step):
        for j in range(0, h, step):
            win = frame[max(j - half, 0):min(j + half, h - 1) + 1, max(i - half, 0):min(i + half, w - 1) + 1].astype(np.float32).reshape(-1)      # ny outer, nx inner
            total, total_sq = np.add.accumulate(win, dtype=np.float32)[-1], np.add.accumulate(win * win, dtype=np.float32)[-1]                  # sequential folds
            count = f32(win.size)                                                       # (a count of ones is exact)
            mean = total / count
            if (total_sq / count) - (mean * mean) > f32(3.0):
                out.append((i, j))
    return np.array(out, dtype=np.float32).reshape(-1, 2)


def inside(p, w, h):
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (p[..., 0] >= f32(0)) & (p[..., 0] < f32(w)) & (p[..., 1] >= f32(0)) & (p[..., 1] < f32(h))


def flow_pyrlk(frames, pairs, features=None):
    """gfw_flow_pyrlk: frames u8 [n][h][w]; pairs [(a, b)]; features one f32 [..][2] array per frame, or None for the grid mode.  -> dict of next f32 [raw][2],
    status u8 [raw], iters int32 [raw][4], pair_first int32 [n_pairs + 1], points_a / points_b f32 [kept][2] — in the grid mode also grid_points f32 [n][nodes][2]
    (kept nodes first, then zeros) and grid_counts int32 [n], and every pair has `nodes` raw slots (the unused ones: next 0, status 0, iters -1)."""
    frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    h, w = frames[0].shape
    pyr = {}
    out = {}
    slots = None
    if features is None:
        _, _, cols, rows = grid_dims(w, h)
        slots = cols * rows
        features = [grid_points(f) for f in frames]
        out["grid_points"] = np.zeros((len(frames), slots, 2), dtype=np.float32)
        for k, p in enumerate(features):
            out["grid_points"][k, :len(p)] = p
        out["grid_counts"] = np.array([len(p) for p in features], dtype=np.int32)
    nxt, status, iters, first, pa, pb = [], [], [], [0], [], []
    for a, b in pairs:
        for f in (a, b):
            if f not in pyr:
                pyr[f] = pyramid(frames[f])
        feats = np.asarray(features[a], dtype=np.float32).reshape(-1, 2)
        kept = 0
        for k in range(len(feats) if slots is None else slots):
            if k < len(feats):
                n, st, it = track(pyr[a], pyr[b], feats[k, 0], feats[k, 1])
            else:
                n, st, it = (f32(0), f32(0)), 0, [-1] * 4
            nxt.append(n); status.append(st); iters.append(it)
            if st == 1 and inside(np.array(n, dtype=np.float32), w, h):
                pa.append(feats[k]); pb.append(n); kept += 1
        first.append(first[-1] + kept)
    out.update(next=np.array(nxt, dtype=np.float32).reshape(-1, 2), status=np.array(status, dtype=np.uint8), iters=np.array(iters, dtype=np.int32).reshape(-1, 4),
               pair_first=np.array(first, dtype=np.int32), points_a=np.array(pa, dtype=np.float32).reshape(-1, 2), points_b=np.array(pb, dtype=np.float32).reshape(-1, 2))
    return out
