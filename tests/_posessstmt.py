"""Host statement of the essential-matrix pose estimation (pose methods 0 `PoseFindEssentialMat` and 2 `PoseEightPoint` of estimate_pose/mod.rs:27-36) — the checker
of gfw_pose_essential.  Test infrastructure: independent of the device code; not part of the product package.

The reference's two methods hand the undistorted points (`undistort_points_for_optical_flow`, cpu_undistort.rs:642-650) to solvers that are NOT in the reference tree:
OpenCV's findEssentialMat / recoverPose (LMedS) and the `arrsac` / `eight-point` crates.  Neither is reproduced.  What is stated here, operation by operation, is the
published scheme both stand on — the eight-point fit of an essential matrix on unit bearings inside a RANSAC loop, the Sampson distance as its inlier test, a refit on
the best round's inliers, the decomposition into two rotations and the positive-depth test — with THE DRAWS AS DATA.  This file is pinned only by itself and by what it
is for: tests/test_pose_essential_statement.py holds it to recovering a planted camera motion before anything is compared with it.

  prepare    one lens inverse per point (both frames), as tests/_posestmt.prepare takes it: the oracle's undistort_points of `point / flow * video` under the identity
             rotation; (-1e6, -1e6) where the inverse is None (cpu_undistort.rs:855), which takes part like any other point.  The f32 (x, y) give the f64
             normalised point (x, y, 1) and its unit bearing (eight_point.rs:29-34, rs_sync.rs:135-136)
  fit        M = sum over a round's 8 points of kron(b2, b1) kron(b2, b1)^T, folded in draw order; E = the eigenvector of M's smallest eigenvalue (the first of equal
             ones) by a cyclic Jacobi iteration: SWEEPS9 sweeps, (p, q) in row order, a rotation skipped where the off-diagonal is exactly 0
  score      a point is an inlier where the squared Sampson distance of the normalised points under E is <= the threshold
  pick       the first round of maximal count; its inliers in point order; M over them; one Jacobi solve; the SVD of E through the Jacobi eigenvectors of E^T E
             (SWEEPS3 sweeps); R = U W V^T and U W^T V^T with U = [u1 u2 u1 x u2], V = [v1 v2 v1 x v2] (both of determinant +1); per rotation and sign of
             t = +-u3 the inliers whose two depths are positive; the rotation of the higher count wins, equal counts go to the larger trace, then to the first

Arithmetic: float64 numpy arrays, one rounding per written operator (+ - * / sqrt only), batched over rounds (elementwise operations round like scalar ones).
"""
import numpy as np

import _oracle as O

f32 = np.float32
NONE_PT = f32(-1000000.0)                                                             # cpu_undistort.rs:855
SWEEPS9, SWEEPS3 = 10, 8
BIG = 1e150                                                                           # |theta| from which theta * theta would overflow: t = 1 / (2 theta)
IDENT = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])


class Camera:
    """What a call shares: the lens (a tests/_zoomstmt.Clip supplies KernelParams and the lens ids), the video and optical-flow sizes, K, the RANSAC settings."""

    def __init__(self, clip, flow_size, num_iters=200, inlier_threshold=1e-6, min_front=10):
        self.clip, self.video, self.flow = clip, tuple(clip.size), tuple(flow_size)
        self.kp = clip.kernel_params()
        self.kp.lens_correction_amount = 1.0
        self.K = np.array([[float(self.kp.f[0]), 0.0, float(self.kp.c[0])], [0.0, float(self.kp.f[1]), float(self.kp.c[1])], [0.0, 0.0, 1.0]])
        self.num_iters, self.inlier_threshold, self.min_front = int(num_iters), float(inlier_threshold), int(min_front)


def prepare(cam, points_a, points_b):
    """-> x [n][4] f32: the undistorted (x1, y1, x2, y2) of one pair"""
    a, b = np.asarray(points_a, dtype=np.float32).reshape(-1, 2), np.asarray(points_b, dtype=np.float32).reshape(-1, 2)
    n = len(a)
    out = np.zeros((n, 4), dtype=np.float32)
    if n:
        size, video = np.array(cam.flow, dtype=np.float32), np.array(cam.video, dtype=np.float32)
        ident = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1]], dtype=np.float32)
        for k, pts in enumerate((a, b)):
            px = ((pts / size) * video).astype(np.float32)
            out[:, 2 * k:2 * k + 2] = O.undistort_points(cam.kp, cam.clip.model, cam.clip.digital, ident, points=px)
    return out


def bearing(x, y):
    """the unit bearing of the normalised point (x, y, 1): [..][3]"""
    n = np.sqrt(((x * x) + (y * y)) + 1.0)
    return np.stack([x / n, y / n, 1.0 / n], axis=-1)


def moment(x):
    """x [B][P][4] f64 -> M [B][9][9]: the sum of kron(b2, b1) kron(b2, b1)^T folded from 0.0 in list order"""
    b1, b2 = bearing(x[..., 0], x[..., 1]), bearing(x[..., 2], x[..., 3])
    a = np.stack([b2[..., i] * b1[..., j] for i in range(3) for j in range(3)], axis=-1)      # [B][P][9]
    M = np.zeros((x.shape[0], 9, 9))
    for k in range(x.shape[1]):
        M = M + (a[:, k, :, None] * a[:, k, None, :])
    return M


def jacobi(A, sweeps):
    """cyclic Jacobi of symmetric A [B][n][n] -> (diagonal [B][n], V [B][n][n], columns the eigenvectors)"""
    A = np.array(A, dtype=np.float64)
    B, n = A.shape[0], A.shape[1]
    V = np.tile(np.eye(n), (B, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[:, p, q].copy()
                    go = apq != 0.0
                    theta = (A[:, q, q] - A[:, p, p]) / (apq + apq)
                    mag = np.abs(theta)
                    t = np.where(mag >= BIG, 1.0 / (theta + theta), np.where(theta >= 0.0, 1.0, -1.0) / (mag + np.sqrt((theta * theta) + 1.0)))
                    c = 1.0 / np.sqrt((t * t) + 1.0)
                    s = t * c
                    for k in range(n):
                        if k != p and k != q:
                            akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                            A[:, k, p] = A[:, p, k] = np.where(go, (c * akp) - (s * akq), akp)
                            A[:, k, q] = A[:, q, k] = np.where(go, (s * akp) + (c * akq), akq)
                    A[:, p, p] = np.where(go, A[:, p, p] - (t * apq), A[:, p, p])
                    A[:, q, q] = np.where(go, A[:, q, q] + (t * apq), A[:, q, q])
                    A[:, p, q] = A[:, q, p] = np.where(go, 0.0, apq)
                    for k in range(n):
                        vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                        V[:, k, p] = np.where(go, (c * vkp) - (s * vkq), vkp)
                        V[:, k, q] = np.where(go, (s * vkp) + (c * vkq), vkq)
    return np.stack([A[:, i, i] for i in range(n)], axis=1), V


def null_vector(M):
    """E [B][9]: the eigenvector of the smallest eigenvalue of M [B][9][9], the first of equal ones"""
    d, V = jacobi(M, SWEEPS9)
    low, e = d[:, 0].copy(), V[:, :, 0].copy()
    for i in range(1, 9):
        c = d[:, i] < low
        low, e = np.where(c, d[:, i], low), np.where(c[:, None], V[:, :, i], e)
    return e


def sampson(E, x):
    """the squared Sampson distance of the points x [B][P][4] f64 under E [B][9] -> [B][P]"""
    e = [E[:, i, None] for i in range(9)]
    x1, y1, x2, y2 = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    with np.errstate(all="ignore"):
        l0, l1, l2 = ((e[0] * x1) + (e[1] * y1)) + e[2], ((e[3] * x1) + (e[4] * y1)) + e[5], ((e[6] * x1) + (e[7] * y1)) + e[8]       # E x1
        m0, m1 = ((e[0] * x2) + (e[3] * y2)) + e[6], ((e[1] * x2) + (e[4] * y2)) + e[7]                                               # E^T x2
        r = ((x2 * l0) + (y2 * l1)) + l2
        return (r * r) / ((((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1))


def cross(a, b):
    return np.array([(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])])


def rotations_of(E):
    """E [9] -> (Ra [9], Rb [9], t [3]): U W V^T, U W^T V^T and u3"""
    with np.errstate(all="ignore"):
        G = np.zeros((1, 3, 3))
        for j in range(3):
            for k in range(j, 3):
                G[0, j, k] = G[0, k, j] = ((E[j] * E[k]) + (E[3 + j] * E[3 + k])) + (E[6 + j] * E[6 + k])
        d, V = jacobi(G, SWEEPS3)
        lam, cols = [d[0, i] for i in range(3)], [V[0, :, i].copy() for i in range(3)]
        for i, j in ((0, 1), (1, 2), (0, 1)):                                         # descending, a swap only where strictly larger
            if lam[j] > lam[i]:
                lam[i], lam[j], cols[i], cols[j] = lam[j], lam[i], cols[j], cols[i]
        v1, v2 = cols[0], cols[1]
        v3 = cross(v1, v2)
        us = []
        for v in (v1, v2):
            w = np.array([((E[3 * i] * v[0]) + (E[3 * i + 1] * v[1])) + (E[3 * i + 2] * v[2]) for i in range(3)])
            us.append(w / np.sqrt(((w[0] * w[0]) + (w[1] * w[1])) + (w[2] * w[2])))
        u1, u2 = us
        u3 = cross(u1, u2)
        Ra = np.array([((u2[i] * v1[j]) - (u1[i] * v2[j])) + (u3[i] * v3[j]) for i in range(3) for j in range(3)])
        Rb = np.array([((u1[i] * v2[j]) - (u2[i] * v1[j])) + (u3[i] * v3[j]) for i in range(3) for j in range(3)])
    return Ra, Rb, u3


def front_counts(R, t, x):
    """the points x [P][4] f64 whose two depths under (R, t) are positive, and under (R, -t) -> (count, count)"""
    x1, y1, x2, y2 = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    with np.errstate(all="ignore"):
        a0, a1, a2 = ((R[0] * x1) + (R[1] * y1)) + R[2], ((R[3] * x1) + (R[4] * y1)) + R[5], ((R[6] * x1) + (R[7] * y1)) + R[8]
        aa, ab, bb = ((a0 * a0) + (a1 * a1)) + (a2 * a2), ((a0 * x2) + (a1 * y2)) + a2, ((x2 * x2) + (y2 * y2)) + 1.0
        at, bt = ((a0 * t[0]) + (a1 * t[1])) + (a2 * t[2]), ((x2 * t[0]) + (y2 * t[1])) + t[2]
        n1, n2 = (ab * bt) - (at * bb), (aa * bt) - (ab * at)                          # the depths' numerators: z1 = n1 / det, z2 = n2 / det, det = aa bb - ab^2 >= 0
    return int(((n1 > 0.0) & (n2 > 0.0)).sum()), int(((n1 < 0.0) & (n2 < 0.0)).sum())


def quat_of(R):
    """R [9] f64 -> (w, i, j, k) f32: the four-branch form, sqrt only"""
    with np.errstate(all="ignore"):
        tr = (R[0] + R[4]) + R[8]
        if tr > 0.0:
            s = np.sqrt(tr + 1.0) * 2.0
            q = [0.25 * s, (R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s]
        elif R[0] > R[4] and R[0] > R[8]:
            s = np.sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0
            q = [(R[7] - R[5]) / s, 0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s]
        elif R[4] > R[8]:
            s = np.sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0
            q = [(R[2] - R[6]) / s, (R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s]
        else:
            s = np.sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0
            q = [(R[3] - R[1]) / s, (R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s]
    return np.array(q, dtype=np.float64).astype(np.float32)


def decompose(E, x, min_front):
    """the refit E [9] over the inliers x [P][4] f64 -> (R [9], front, found)"""
    Ra, Rb, t = rotations_of(E)
    sa, sb = max(front_counts(Ra, t, x)), max(front_counts(Rb, t, x))
    tra, trb = (Ra[0] + Ra[4]) + Ra[8], (Rb[0] + Rb[4]) + Rb[8]
    use_b = sb > sa or (sb == sa and trb > tra)
    R, front = (Rb, sb) if use_b else (Ra, sa)
    return R, front, front >= min_front


def estimate_pair(cam, points_a, points_b, octets):
    """One pair -> dict(rotation [3][3] f64, quat [4] f32, essential [9] f64, best (inliers, round, front, found), round_inliers [iters], round_fits [iters][9],
    inlier_idx)"""
    x = prepare(cam, points_a, points_b).astype(np.float64)
    n, iters = len(x), cam.num_iters
    counts, fits = np.zeros(iters, dtype=np.int32), np.zeros((iters, 9))
    R, E, best, keep = IDENT.copy(), np.zeros(9), (0, 0 if iters else -1, 0, 0), np.zeros(0, dtype=np.int64)
    if n >= 8 and iters:
        idx = np.asarray(octets, dtype=np.int64).reshape(iters, 8)
        fits = null_vector(moment(x[idx]))
        inl = sampson(fits, np.tile(x[None], (iters, 1, 1))) <= cam.inlier_threshold
        counts = inl.sum(axis=1).astype(np.int32)
        rnd = int(np.argmax(counts))                                                  # the first of the maximal rounds
        keep = np.flatnonzero(inl[rnd])
        best = (int(counts[rnd]), rnd, 0, 0)
        if best[0] >= 8:
            E = null_vector(moment(x[keep][None]))[0]
            Rw, front, found = decompose(E, x[keep], cam.min_front)
            best = (best[0], rnd, front, int(found))
            if found:
                R = Rw
    return dict(rotation=R.reshape(3, 3), quat=quat_of(R), essential=E, best=best, round_inliers=counts, round_fits=fits, inlier_idx=keep)


def estimate(cam, pairs, octets):
    """gfw_pose_essential's outputs for pairs [(points_a, points_b)] -> (quats [n][4] f32, rotations [n][3][3], essential [n][9], best [n][4], round_inliers
    [n][iters], round_fits [n][iters][9])"""
    out = [estimate_pair(cam, a, b, octets[p]) for p, (a, b) in enumerate(pairs)]
    n, iters = len(pairs), cam.num_iters
    stack = lambda key, shape, dt: np.array([o[key] for o in out], dtype=dt).reshape(shape)
    return (stack("quat", (n, 4), np.float32), stack("rotation", (n, 3, 3), np.float64), stack("essential", (n, 9), np.float64), stack("best", (n, 4), np.int32),
            stack("round_inliers", (n, iters), np.int32), stack("round_fits", (n, iters, 9), np.float64))
