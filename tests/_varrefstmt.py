"""TEST INFRASTRUCTURE: the statement gfw_flow_dis_refined is held to — tests/_disstmt.py's DIS dense flow (imported, not edited) with the variational refinement the
reference's DISOpticalFlow_PRESET_FAST runs on every pyramid level (5 iterations): the Brox-style refinement (Brox, Bruhn, Papenberg, Weickert, "High Accuracy
Optical Flow Estimation Based on a Theory for Warping") as Kroeger et al. use it.  OpenCV's source is not part of the reference tree and OpenCV is not a dependency:
this is one more builder-written restatement after the published scheme, held to what refinement is for by tests/test_varref_statement.py before anything is
compared with it.  The defaults (alpha 20, delta 5, gamma 10, 5 fixed-point and 5 SOR iterations, omega 1.6; zeta 0.1 and eps 0.001 are fixed) are the values
OpenCV's DIS implementation sets to the builder's best knowledge; nothing in the tree confirms them.

Where: once per level and pair, directly after Level.dense(u); the next finer level's start values, and at the finest level the nodes and `flow`, read the refined
field.  In: the level's images A, B (u8 [h][w]), the field U f32 [h][w][2] = (u, v), and the configuration.  fixed_point_iters = 0 returns U itself.

EVERYTHING IS f32 AND EVERY WRITTEN OPERATOR ROUNDS ONCE (+ - * / and sqrt correctly rounded, nothing contracted); a parenthesis is evaluated first, and what is
written without one runs LEFT TO RIGHT.  c(i, n) = min(max(i, 0), n - 1).
  once per level:
    I0 = f32(A);  I1w = f32(_disstmt.sample(B, x, y, u, v)) * 0.03125          (the 14-bit fixed-point sampler, edge replicated; the product is exact)
    avg = (I0 + I1w) * 0.5;  Iz = I1w - I0
    dx(a)(x, y) = (a(c(x + 1, w), y) - a(c(x - 1, w), y)) * 0.5;  dy alike over rows.  The indices are clamped at EVERY application: Ixx(0, y) = (Ix(1, y) - Ix(0, y))
    0.5 with Ix(0, y) = (avg(1, y) - avg(0, y)) 0.5.
    Ix = dx(avg), Iy = dy(avg), Ixx = dx(Ix), Ixy = dy(Ix), Iyy = dy(Iy), Ixz = dx(Iz), Iyz = dy(Iz);  du = dv = 0
  per fixed-point iteration, zeta = 0.1, eps2 = 0.000001:
    brightness   n = Ix Ix + Iy Iy + zeta;  k = Iz + Ix du + Iy dv;  wt = (delta / sqrt(k k / n + eps2)) / n
                 a11 = wt Ix Ix, a12 = wt Ix Iy, a22 = wt Iy Iy, b1 = -(wt Iz Ix), b2 = -(wt Iz Iy)
    gradient     nx = Ixx Ixx + Ixy Ixy + zeta;  ny = Iyy Iyy + Ixy Ixy + zeta;  kx = Ixz + Ixx du + Ixy dv;  ky = Iyz + Ixy du + Iyy dv
                 wg = gamma / sqrt((kx kx / nx + ky ky / ny) + eps2)
                 a11 = a11 + wg (Ixx Ixx / nx + Ixy Ixy / ny);  a12 = a12 + wg (Ixx Ixy / nx + Ixy Iyy / ny);  a22 = a22 + wg (Ixy Ixy / nx + Iyy Iyy / ny)
                 b1 = b1 - wg (Ixx Ixz / nx + Ixy Iyz / ny);  b2 = b2 - wg (Ixy Ixz / nx + Iyy Iyz / ny)       (p q / r is (p q) / r)
    smoothness   P = u + du, Q = v + dv;  fx(P)(x, y) = P(x + 1, y) - P(x, y), 0 in the last column;  fy(P)(x, y) = P(x, y + 1) - P(x, y), 0 in the last row
                 s = alpha / sqrt(fx(P) fx(P) + fy(P) fy(P) + fx(Q) fx(Q) + fy(Q) fy(Q) + eps2)
                 wr(x, y) = (s(x, y) + s(x + 1, y)) 0.5, 0 in the last column;  wd(x, y) = (s(x, y) + s(x, y + 1)) 0.5, 0 in the last row
                 wl(x, y) = wr(x - 1, y), 0 in the first column;  wu(x, y) = wd(x, y - 1), 0 in the first row: no link leaves the level
    THE FOUR LINKS ARE ALWAYS TAKEN IN THE ORDER right, left, down, up; a link that does not exist has the weight 0 and the pixel itself as its neighbour:
                 ws = wr + wl + wd + wu;  A11 = a11 + ws;  A22 = a22 + ws
                 B1 = b1 + (wr (u_r - u) + wl (u_l - u) + wd (u_d - u) + wu (u_u - u));  B2 = b2 + the same of v        (u, v: the level's field, without du, dv)
    sor_iters times, the colour (x + y) even first, then odd; within a colour the order is free, because the four neighbours have the other colour:
                 su = wr du_r + wl du_l + wd du_d + wu du_u;  sv alike of dv
                 du' = du + omega ((su + B1 - a12 dv) / A11 - du)
                 dv' = dv + omega ((sv + B2 - a12 du') / A22 - dv)                                                        (the pixel's own NEW du)
  U_refined = (u + du, v + dv)

What the statement asserts while it runs:
  every index lies inside the level: each is formed with c(., n), or under a mask that names the last / first column or row.
  every square-root argument is >= eps2 > 0: it is eps2 added LAST to a sum of squares and quotients of squares by n, nx, ny >= zeta > 0 — all >= 0, and round-to-
      nearest keeps x + eps2 >= eps2 for x >= 0.
  A11 > 0 and A22 > 0: a11 = (wt Ix) Ix >= 0 with wt > 0 (the rounded product of a square with a positive number keeps its sign or is 0), the gradient term adds
      wg times quotients of squares, >= 0.  A level has sides >= 8, so a pixel has at least two links, and a link's weight is the mean of two s with
      s >= alpha / sqrt(4 (2 x 16384)^2 + eps2) > 0 wherever the field stays within the sampler's clamp of +-16384: ws > 0 and A = a + ws > 0.
  every result is finite: the denominators are A11, A22 > 0, n, nx, ny >= zeta and square roots >= eps = 0.001.
The traces (a list per pair) receive (level, fixed-point iteration, SOR iteration, colour, the boolean mask of the pixels updated)."""
import collections

import numpy as np

import _disstmt as DS
import _flowstmt as FS

f32 = np.float32
Cfg = collections.namedtuple("Cfg", "fixed_point_iters sor_iters alpha delta gamma omega")
DEFAULT = Cfg(5, 5, 20.0, 5.0, 10.0, 1.6)
ZETA, EPS2, HALF = f32(0.1), f32(0.000001), f32(0.5)


def _cl(i, n):
    i = np.minimum(np.maximum(i, 0), n - 1)
    assert (i >= 0).all() and (i < n).all()
    return i


def _dx(a):
    x = np.arange(a.shape[1])
    return (a[:, _cl(x + 1, a.shape[1])] - a[:, _cl(x - 1, a.shape[1])]) * HALF


def _dy(a):
    y = np.arange(a.shape[0])
    return (a[_cl(y + 1, a.shape[0]), :] - a[_cl(y - 1, a.shape[0]), :]) * HALF


def _sqrt(a):
    assert (a >= EPS2).all()
    return np.sqrt(a)


def _nb(a, ox, oy):
    """a at the neighbour (x + ox, y + oy), the pixel itself where the link does not exist"""
    h, w = a.shape
    return a[_cl(np.arange(h) + oy, h)[:, None], _cl(np.arange(w) + ox, w)[None, :]]


def refine(A, B, U, cfg, trace=None, level=0):
    """one level of one pair: A, B u8 [h][w], U f32 [h][w][2] -> the refined field f32 [h][w][2]"""
    if cfg.fixed_point_iters == 0:
        return U
    h, w = A.shape
    assert U.shape == (h, w, 2) and U.dtype == f32 and h >= 8 and w >= 8
    alpha, delta, gamma, omega = f32(cfg.alpha), f32(cfg.delta), f32(cfg.gamma), f32(cfg.omega)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = U[..., 0], U[..., 1]
    I0 = A.astype(f32)
    I1w = DS.sample(B, xx, yy, u, v).astype(f32) * f32(0.03125)
    avg = (I0 + I1w) * HALF
    Iz = I1w - I0
    Ix, Iy = _dx(avg), _dy(avg)
    Ixx, Ixy, Iyy, Ixz, Iyz = _dx(Ix), _dy(Ix), _dy(Iy), _dx(Iz), _dy(Iz)
    du, dv = np.zeros((h, w), f32), np.zeros((h, w), f32)
    zero = np.zeros((h, w), f32)
    last_col, last_row, first_col, first_row = xx == w - 1, yy == h - 1, xx == 0, yy == 0
    colour = (xx + yy) & 1
    n = ((Ix * Ix) + (Iy * Iy)) + ZETA
    nx = ((Ixx * Ixx) + (Ixy * Ixy)) + ZETA
    ny = ((Iyy * Iyy) + (Ixy * Ixy)) + ZETA
    with np.errstate(all="raise", under="ignore"):
        for fp in range(cfg.fixed_point_iters):
            k = (Iz + (Ix * du)) + (Iy * dv)
            wt = (delta / _sqrt(((k * k) / n) + EPS2)) / n
            a11, a12, a22 = (wt * Ix) * Ix, (wt * Ix) * Iy, (wt * Iy) * Iy
            b1, b2 = -((wt * Iz) * Ix), -((wt * Iz) * Iy)
            kx = (Ixz + (Ixx * du)) + (Ixy * dv)
            ky = (Iyz + (Ixy * du)) + (Iyy * dv)
            wg = gamma / _sqrt((((kx * kx) / nx) + ((ky * ky) / ny)) + EPS2)
            a11 = a11 + (wg * (((Ixx * Ixx) / nx) + ((Ixy * Ixy) / ny)))
            a12 = a12 + (wg * (((Ixx * Ixy) / nx) + ((Ixy * Iyy) / ny)))
            a22 = a22 + (wg * (((Ixy * Ixy) / nx) + ((Iyy * Iyy) / ny)))
            b1 = b1 - (wg * (((Ixx * Ixz) / nx) + ((Ixy * Iyz) / ny)))
            b2 = b2 - (wg * (((Ixy * Ixz) / nx) + ((Iyy * Iyz) / ny)))
            P, Q = u + du, v + dv
            fxP, fyP = np.where(last_col, zero, _nb(P, 1, 0) - P), np.where(last_row, zero, _nb(P, 0, 1) - P)
            fxQ, fyQ = np.where(last_col, zero, _nb(Q, 1, 0) - Q), np.where(last_row, zero, _nb(Q, 0, 1) - Q)
            s = alpha / _sqrt(((((fxP * fxP) + (fyP * fyP)) + (fxQ * fxQ)) + (fyQ * fyQ)) + EPS2)
            wr = np.where(last_col, zero, (s + _nb(s, 1, 0)) * HALF)
            wd = np.where(last_row, zero, (s + _nb(s, 0, 1)) * HALF)
            wl = np.where(first_col, zero, _nb(wr, -1, 0))
            wu = np.where(first_row, zero, _nb(wd, 0, -1))
            ws = ((wr + wl) + wd) + wu
            A11, A22 = a11 + ws, a22 + ws
            assert (A11 > 0).all() and (A22 > 0).all()
            B1 = b1 + ((((wr * (_nb(u, 1, 0) - u)) + (wl * (_nb(u, -1, 0) - u))) + (wd * (_nb(u, 0, 1) - u))) + (wu * (_nb(u, 0, -1) - u)))
            B2 = b2 + ((((wr * (_nb(v, 1, 0) - v)) + (wl * (_nb(v, -1, 0) - v))) + (wd * (_nb(v, 0, 1) - v))) + (wu * (_nb(v, 0, -1) - v)))
            for it in range(cfg.sor_iters):
                for col in (0, 1):
                    on = colour == col
                    su = (((wr * _nb(du, 1, 0)) + (wl * _nb(du, -1, 0))) + (wd * _nb(du, 0, 1))) + (wu * _nb(du, 0, -1))
                    sv = (((wr * _nb(dv, 1, 0)) + (wl * _nb(dv, -1, 0))) + (wd * _nb(dv, 0, 1))) + (wu * _nb(dv, 0, -1))
                    du2 = du + (omega * ((((su + B1) - (a12 * dv)) / A11) - du))
                    dv2 = dv + (omega * ((((sv + B2) - (a12 * du2)) / A22) - dv))
                    du, dv = np.where(on, du2, du), np.where(on, dv2, dv)
                    if trace is not None:
                        trace.append((level, fp, it, col, on.copy()))
            assert np.isfinite(du).all() and np.isfinite(dv).all()
    out = np.stack([u + du, v + dv], axis=2).astype(f32)
    assert np.isfinite(out).all()
    return out


def dense_flow_refined(pa, pb, finest, cfg, trace=None):
    """_disstmt.dense_flow with `refine` after every level's dense field; ``trace`` receives the SOR colours' masks"""
    U = None
    for l in range(len(pa) - 1, finest - 1, -1):
        L = DS.Level(pa[l], pb[l])
        if U is None:
            u0 = np.zeros((L.nx * L.ny, 2), f32)
        else:
            u0 = (f32(2) * DS.bilinear(U, ((DS.STRIDE * L.pi + 4).astype(f32) * f32(0.5)) - f32(0.25), ((DS.STRIDE * L.pj + 4).astype(f32) * f32(0.5)) - f32(0.25))).astype(f32)
        u = u0
        for nb in ([], [(-1, 0), (0, -1)], [(1, 0), (0, 1)]):
            u = L.run_pass(u0, u, nb)
        U = refine(pa[l], pb[l], L.dense(u), cfg, trace, l)
    return U


def flow_dis_refined(frames, pairs, finest, cfg, traces=None):
    """gfw_flow_dis_refined: the dictionary of _disstmt.flow_dis, its fields refined on every level"""
    frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    h, w = frames[0].shape
    assert finest in (1, 2) and DS.coarsest_scale(w, h) >= finest and max(w, h) <= DS.SIDE_MAX
    _, _, cols, rows = FS.grid_dims(w, h)
    nodes = [FS.grid_points(f) for f in frames]
    out = {"grid_points": np.zeros((len(frames), cols * rows, 2), f32), "grid_counts": np.array([len(p) for p in nodes], dtype=np.int32)}
    for k, p in enumerate(nodes):
        out["grid_points"][k, :len(p)] = p
    pyr, flows, first, pa, pb = {}, [], [0], [], []
    for a, b in pairs:
        for f in (a, b):
            if f not in pyr:
                pyr[f] = DS.pyramid(frames[f])
        tr = None if traces is None else []
        U = dense_flow_refined(pyr[a], pyr[b], finest, cfg, tr)
        if traces is not None:
            traces.append(tr)
        flows.append(U)
        pa.append(nodes[a]); pb.append(DS.nodes_to(U, nodes[a], finest))
        first.append(first[-1] + len(nodes[a]))
    fw, fh = DS.level_sizes(w, h)[finest]
    out.update(flow=np.array(flows, dtype=f32).reshape(len(pairs), fh, fw, 2), pair_first=np.array(first, dtype=np.int32),
               points_a=np.concatenate(pa + [np.zeros((0, 2), f32)]).astype(f32), points_b=np.concatenate(pb + [np.zeros((0, 2), f32)]).astype(f32))
    return out
