"""TEST INFRASTRUCTURE: the statement gfw_flow_dis is held to — the DIS dense optical flow (Kroeger, Timofte, Dai, Van Gool, "Fast Optical Flow using Dense Inverse
Search") with the parameters of the reference's DISOpticalFlow_PRESET_FAST (src/core/synchronization/optical_flow/opencv_dis.rs:59): patch 8, patch stride 4, 16
descent iterations, finest scale 2, mean-normalised patches, spatial propagation — sampled at the grid nodes of opencv_dis.rs:62-119.  OpenCV's source is not part of
the reference tree and OpenCV is not a dependency: this is a builder-written statement after the published scheme, held to its purpose by
tests/test_dis_statement.py before anything is compared with it.  VARIATIONAL REFINEMENT IS NOT PART OF IT (the preset runs 5 iterations; `variational_iters` must be
0).  OpenCV's spatial propagation is a raster sweep whose result depends on its own thread count; it is not reproduced: the propagation below is three synchronous
passes, so no result depends on an order of execution.

Every sum over a patch's 64 pixels is an INTEGER, so a parallel reduction may take any order and still equal this to the bit:
  frames    n u8 gray planes of one width x height.
  scales    coarsest = min(int(log2(max(w, h) / 32) + 0.5), int(log2(min(w, h) / 8))); levels coarsest .. finest are processed, finest 1 or 2; coarsest < finest is
            refused.  Level l + 1 has sides w_l // 2, h_l // 2 and the pixels (a + b + c + d + 2) >> 2 of the 2 x 2 blocks at (2x, 2y): an odd last column or row is
            not read.  The coarsest level's smaller side is >= 8, so every level holds a patch.
  per level and pair (A, B), sides w x h:
    gradients  Ix(x, y) = A(min(x + 1, w - 1), y) - A(max(x - 1, 0), y) (the edge replicated), Iy alike: integers in [-255, 255], TWICE the derivative.
    patches    origins (4i, 4j), i < (w - 8) // 4 + 1 = nx, j < (h - 8) // 4 + 1 = ny; patch index j nx + i.  Sx = sum Ix, Sy, Sxx = sum Ix Ix, Sxy, Syy (exact).
    system     the mean-normalised 2 x 2 system times 64, formed in integers: Hxx = f32(64 Sxx - Sx Sx), Hxy = f32(64 Sxy - Sx Sy), Hyy = f32(64 Syy - Sy Sy), one
               conversion each; det = Hxx Hyy - Hxy Hxy.  A patch with det <= 2^24 is never descended: it has its start value in every pass.
    sample     B at the patch pixel (x, y) displaced by u: f = floor(u), a = u - f, the integer part min(max(f, -16384), 16384) cast to int (sides are <= 8192: beyond
               that every index is clamped anyway, and no cast outside the int range is made); weights of 14 bits as tests/_flowstmt.py's: w00 = rint(((1-ax)(1-ay))
               16384), w01 = rint((ax (1-ay)) 16384), w10 = rint(((1-ax) ay) 16384), w11 = 16384 - w00 - w01 - w10; columns clamp(x + ix, 0, w - 1) and
               clamp(x + ix + 1, 0, w - 1), rows alike — the edge replicated, which IS the position clamped into the level; Bs = (sum w B + 256) >> 9: 5 fraction
               bits, 0 .. 8160.  d = Bs - 32 A, |d| <= 8160.
    evaluate   at a value u: Sd = sum d, Sdd = sum d d (<= 64 8160^2 < 2^32), Sxd = sum Ix d, Syd = sum Iy d (< 2^28), int64;
               ssd = f32(64 Sdd - Sd Sd) (64 times the mean-normalised SSD; < 2^38), bx = f32(64 Sxd - Sx Sd), by = f32(64 Syd - Sy Sd).
    step       idet = 1 / det; dx = ((Hyy bx) - (Hxy by)) idet, dy = ((Hxx by) - (Hxy bx)) idet; the proposal is u - (0.03125 dx, 0.03125 dy): H and b carry 64 and d
               carries 32, so this is u - H^-1 b with the integer gradients as they are.  Those are twice the derivative, so the step is HALF the Gauss-Newton
               step: a damped descent.  (The full step, 0.0625, was tried on the scenes of tests/test_dis_statement.py: worst node 0.403 px instead of 0.376 at the
               finest scale 2 and 0.263 px instead of 0.123 at 1.)
    descent    evaluate u; up to 16 times: evaluate the proposal, accept it only if its ssd is strictly smaller, else stop.
    start      u0 = 0 at the coarsest level, else 2 bilinear(U_{l+1}, (x + 4) 0.5 - 0.25, (y + 4) 0.5 - 0.25) at the patch origin (x, y) (see `bilinear`).
    passes     (a) from u0: descend.  (b) from the patch's pass-(a) value: evaluate it, then the pass-(a) value of the left neighbour (i - 1, j) and then of the top
               neighbour (i, j - 1), taking a strictly smaller ssd each time; descend.  (c) the same from pass (b) with the right and then the bottom neighbour.
               At the end of EACH pass a value with (u - u0).x^2 + (u - u0).y^2 > 64 returns to u0.
    dense      U(x, y), with (xc, yc) = (min(x, 4 (nx - 1) + 7), min(y, 4 (ny - 1) + 7)): over the patches j in max(0, (yc - 4) >> 2) .. min(yc >> 2, ny - 1) (outer),
               i alike (inner): wt = 32 / f32(max(32, |Bs(xc, yc, u) - 32 A(xc, yc)|)) — 1 / max(1, |B - A|) —, sw += wt, sx += wt ux, sy += wt uy from 0;
               U = (sx / sw, sy / sw).
  bilinear  of a field U of sides w x h at (cx, cy): c = min(max(c, 0), n - 1); f = floor(c), a = c - f, i0 = int(f), i1 = min(i0 + 1, n - 1);
            (((1-ax)(1-ay)) U00 + (ax (1-ay)) U01) + ((1-ax) ay) U10) + (ax ay) U11, left to right.
  result    for each node (i, j) the grid keeps in the pair's first frame (tests/_flowstmt.grid_points, unchanged): a = (i, j),
            b = a + 2^finest bilinear(U_finest, (i + 0.5) 2^-finest - 0.5, (j + 0.5) 2^-finest - 0.5).  Every kept node is returned, in grid order
            (opencv_dis.rs:113-117 filters nothing); pair_first is the prefix sum of the first frames' grid counts.
Every f32 operation is a single operation (-ffp-contract=off on the device)."""
import math

import numpy as np

import _flowstmt as FS

f32 = np.float32
PATCH, STRIDE, ITERS = 8, 4, 16
DET_MIN = f32(16777216.0)
FAR2 = f32(64.0)
SIDE_MAX = 8192


def coarsest_scale(width, height):
    return min(int(math.log2(max(width, height) / 32.0) + 0.5), int(math.log2(min(width, height) / 8.0)))


def level_sizes(width, height):
    """-> [(w_l, h_l)] of levels 0 .. coarsest (empty where coarsest < 0)"""
    out = [(width, height)]
    for _ in range(coarsest_scale(width, height)):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def down(img):
    h, w = img.shape
    a = img[:h // 2 * 2, :w // 2 * 2].astype(np.int64)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(frame):
    levels = [np.ascontiguousarray(frame, dtype=np.uint8)]
    for _ in level_sizes(frame.shape[1], frame.shape[0])[1:]:
        levels.append(down(levels[-1]))
    return levels


def _weights(ax, ay):
    na, nb = f32(1) - ax, f32(1) - ay
    w00 = np.rint((na * nb) * f32(16384)).astype(np.int64)
    w01 = np.rint((ax * nb) * f32(16384)).astype(np.int64)
    w10 = np.rint((na * ay) * f32(16384)).astype(np.int64)
    return w00, w01, w10, 16384 - w00 - w01 - w10


def sample(B, x, y, ux, uy):
    """Bs at the integer pixels (x, y) displaced by (ux, uy) (f32), all arrays of one shape"""
    h, w = B.shape
    fx, fy = np.floor(ux), np.floor(uy)
    W = _weights(ux - fx, uy - fy)
    ix = np.minimum(np.maximum(fx, f32(-16384)), f32(16384)).astype(np.int64)
    iy = np.minimum(np.maximum(fy, f32(-16384)), f32(16384)).astype(np.int64)
    c0, c1 = np.clip(x + ix, 0, w - 1), np.clip(x + ix + 1, 0, w - 1)
    r0, r1 = np.clip(y + iy, 0, h - 1), np.clip(y + iy + 1, 0, h - 1)
    for idx, n in ((c0, w), (c1, w), (r0, h), (r1, h)):
        assert (idx >= 0).all() and (idx < n).all()                                  # no index outside the level
    Bi = B.astype(np.int64)
    return (W[0] * Bi[r0, c0] + W[1] * Bi[r0, c1] + W[2] * Bi[r1, c0] + W[3] * Bi[r1, c1] + 256) >> 9


def bilinear(U, cx, cy):
    """U f32 [h][w][2] at the f32 coordinates (cx, cy) -> f32 [..][2]"""
    h, w = U.shape[:2]
    cx = np.minimum(np.maximum(np.asarray(cx, dtype=f32), f32(0)), f32(w - 1))
    cy = np.minimum(np.maximum(np.asarray(cy, dtype=f32), f32(0)), f32(h - 1))
    fx, fy = np.floor(cx), np.floor(cy)
    ax, ay = (cx - fx)[..., None], (cy - fy)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    assert (x0 >= 0).all() and (x1 < w).all() and (y0 >= 0).all() and (y1 < h).all()
    na, nb = f32(1) - ax, f32(1) - ay
    return ((((na * nb) * U[y0, x0]) + ((ax * nb) * U[y0, x1])) + ((na * ay) * U[y1, x0])) + ((ax * ay) * U[y1, x1])


class Level:
    """One level of one pair: the template side (A's patches) and the evaluation against B"""

    def __init__(self, A, B):
        self.A, self.B = A, B
        h, w = A.shape
        self.w, self.h = w, h
        self.nx, self.ny = (w - PATCH) // STRIDE + 1, (h - PATCH) // STRIDE + 1
        Ai = A.astype(np.int64)
        xs, ys = np.arange(w), np.arange(h)
        Ix = Ai[:, np.minimum(xs + 1, w - 1)] - Ai[:, np.maximum(xs - 1, 0)]
        Iy = Ai[np.minimum(ys + 1, h - 1), :] - Ai[np.maximum(ys - 1, 0), :]
        j, i = np.mgrid[0:self.ny, 0:self.nx]
        self.pi, self.pj = i.reshape(-1), j.reshape(-1)
        k = np.arange(64)
        self.px = (STRIDE * self.pi)[:, None] + (k % 8)[None, :]                       # [P][64]
        self.py = (STRIDE * self.pj)[:, None] + (k // 8)[None, :]
        self.Ap, self.Ixp, self.Iyp = Ai[self.py, self.px], Ix[self.py, self.px], Iy[self.py, self.px]
        self.Sx, self.Sy = self.Ixp.sum(axis=1), self.Iyp.sum(axis=1)
        self.Hxx = (64 * (self.Ixp * self.Ixp).sum(axis=1) - self.Sx * self.Sx).astype(f32)
        self.Hxy = (64 * (self.Ixp * self.Iyp).sum(axis=1) - self.Sx * self.Sy).astype(f32)
        self.Hyy = (64 * (self.Iyp * self.Iyp).sum(axis=1) - self.Sy * self.Sy).astype(f32)
        self.det = (self.Hxx * self.Hyy) - (self.Hxy * self.Hxy)
        self.descended = self.det > DET_MIN

    def evaluate(self, u):
        """u f32 [P][2] -> ssd, bx, by f32 [P]"""
        d = sample(self.B, self.px, self.py, u[:, 0:1], u[:, 1:2]) - 32 * self.Ap
        Sd = d.sum(axis=1)
        ssd = (64 * (d * d).sum(axis=1) - Sd * Sd).astype(f32)
        bx = (64 * (self.Ixp * d).sum(axis=1) - self.Sx * Sd).astype(f32)
        by = (64 * (self.Iyp * d).sum(axis=1) - self.Sy * Sd).astype(f32)
        return ssd, bx, by

    def run_pass(self, u0, u_in, neighbours, trace=None):
        """u0 the start values, u_in the values the pass starts from, neighbours [(di, dj)] read from u_in -> the pass's values f32 [P][2]"""
        on = self.descended
        u = u_in.copy()
        with np.errstate(all="ignore"):
            ssd, bx, by = self.evaluate(u)
            for di, dj in neighbours:
                ni, nj = self.pi + di, self.pj + dj
                valid = on & (ni >= 0) & (ni < self.nx) & (nj >= 0) & (nj < self.ny)
                cand = u_in[np.clip(nj, 0, self.ny - 1) * self.nx + np.clip(ni, 0, self.nx - 1)]
                s2, bx2, by2 = self.evaluate(cand)
                take = valid & (s2 < ssd)
                u[take], ssd[take], bx[take], by[take] = cand[take], s2[take], bx2[take], by2[take]
            idet = f32(1) / np.where(on, self.det, f32(1))
            active = on.copy()
            for _ in range(ITERS):
                if not active.any():
                    break
                dx = ((self.Hyy * bx) - (self.Hxy * by)) * idet
                dy = ((self.Hxx * by) - (self.Hxy * bx)) * idet
                prop = np.stack([u[:, 0] - (f32(0.03125) * dx), u[:, 1] - (f32(0.03125) * dy)], axis=1).astype(f32)
                prop[~active] = u[~active]
                s2, bx2, by2 = self.evaluate(prop)
                acc = active & (s2 < ssd)
                u[acc], ssd[acc], bx[acc], by[acc] = prop[acc], s2[acc], bx2[acc], by2[acc]
                active = acc
            ex, ey = u[:, 0] - u0[:, 0], u[:, 1] - u0[:, 1]
            far = on & (((ex * ex) + (ey * ey)) > FAR2)
        if trace is not None:
            trace.extend(int(p) for p in np.flatnonzero(far))
        u[far | ~on] = u0[far | ~on]
        return u

    def dense(self, u):
        """the patch values u f32 [P][2] -> U f32 [h][w][2]"""
        yy, xx = np.mgrid[0:self.h, 0:self.w]
        xc, yc = np.minimum(xx, STRIDE * (self.nx - 1) + 7), np.minimum(yy, STRIDE * (self.ny - 1) + 7)
        ilo, ihi = np.maximum(0, (xc - 4) >> 2), np.minimum(xc >> 2, self.nx - 1)
        jlo, jhi = np.maximum(0, (yc - 4) >> 2), np.minimum(yc >> 2, self.ny - 1)
        sw, sx, sy = np.zeros(xc.shape, f32), np.zeros(xc.shape, f32), np.zeros(xc.shape, f32)
        A32 = 32 * self.A.astype(np.int64)[yc, xc]
        for dj in (0, 1):
            for di in (0, 1):
                pj, pi = jlo + dj, ilo + di
                ok = (pj <= jhi) & (pi <= ihi)
                up = u[np.minimum(pj, jhi) * self.nx + np.minimum(pi, ihi)]
                ux, uy = up[..., 0], up[..., 1]
                diff = np.abs(sample(self.B, xc, yc, ux, uy) - A32)
                wt = f32(32) / np.maximum(32, diff).astype(f32)
                sw = np.where(ok, sw + wt, sw)
                sx = np.where(ok, sx + (wt * ux), sx)
                sy = np.where(ok, sy + (wt * uy), sy)
        return np.stack([sx / sw, sy / sw], axis=2).astype(f32)


def dense_flow(pa, pb, finest, trace=None):
    """the pyramids of a pair's two frames -> U_finest f32 [h_f][w_f][2]; ``trace`` receives (level, pass, patch index) of every return to the start value"""
    U = None
    for l in range(len(pa) - 1, finest - 1, -1):
        L = Level(pa[l], pb[l])
        if U is None:
            u0 = np.zeros((L.nx * L.ny, 2), f32)
        else:
            u0 = (f32(2) * bilinear(U, ((STRIDE * L.pi + 4).astype(f32) * f32(0.5)) - f32(0.25), ((STRIDE * L.pj + 4).astype(f32) * f32(0.5)) - f32(0.25))).astype(f32)
        u = u0
        for name, nb in (("a", []), ("b", [(-1, 0), (0, -1)]), ("c", [(1, 0), (0, 1)])):
            t = None if trace is None else []
            u = L.run_pass(u0, u, nb, t)
            if trace is not None:
                trace.extend((l, name, p) for p in t)
        U = L.dense(u)
    return U


def nodes_to(U, nodes, finest):
    """the kept nodes f32 [n][2] through the finest field -> points_b f32 [n][2]"""
    inv, scale = f32(2.0 ** -finest), f32(2.0 ** finest)
    v = bilinear(U, ((nodes[:, 0] + f32(0.5)) * inv) - f32(0.5), ((nodes[:, 1] + f32(0.5)) * inv) - f32(0.5))
    return (nodes + (scale * v)).astype(f32)


def flow_dis(frames, pairs, finest=2, traces=None):
    """gfw_flow_dis: frames u8 [n][h][w]; pairs [(a, b)] -> dict of grid_points f32 [n][nodes][2] (kept nodes first, then zeros), grid_counts int32 [n], flow f32
    [n_pairs][h_f][w_f][2], pair_first int32 [n_pairs + 1], points_a / points_b f32 [total][2].  ``traces``: a list that receives one trace per pair."""
    frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    h, w = frames[0].shape
    assert finest in (1, 2) and coarsest_scale(w, h) >= finest and max(w, h) <= SIDE_MAX
    _, _, cols, rows = FS.grid_dims(w, h)
    nodes = [FS.grid_points(f) for f in frames]
    out = {"grid_points": np.zeros((len(frames), cols * rows, 2), f32), "grid_counts": np.array([len(p) for p in nodes], dtype=np.int32)}
    for k, p in enumerate(nodes):
        out["grid_points"][k, :len(p)] = p
    pyr = {}
    flows, first, pa, pb = [], [0], [], []
    for a, b in pairs:
        for f in (a, b):
            if f not in pyr:
                pyr[f] = pyramid(frames[f])
        tr = None if traces is None else []
        U = dense_flow(pyr[a], pyr[b], finest, tr)
        if traces is not None:
            traces.append(tr)
        flows.append(U)
        pa.append(nodes[a]); pb.append(nodes_to(U, nodes[a], finest))
        first.append(first[-1] + len(nodes[a]))
    fw, fh = level_sizes(w, h)[finest]
    out.update(flow=np.array(flows, dtype=f32).reshape(len(pairs), fh, fw, 2), pair_first=np.array(first, dtype=np.int32),
               points_a=np.concatenate(pa + [np.zeros((0, 2), f32)]).astype(f32), points_b=np.concatenate(pb + [np.zeros((0, 2), f32)]).astype(f32))
    return out
