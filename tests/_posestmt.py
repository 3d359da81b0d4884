"""Host statement of Almeida pose estimation (src/core/synchronization/estimate_pose/almeida.rs:23-238) — the checker of gfw_pose_almeida.  Test infrastructure:
written from the cited Rust, independent of the device code; not part of the product package.

  prepare          estimate_pose :23-37 (pos, motion) and what `Camera::delta` (:58-68) needs once per point: the lens inverse of `pos * (vw, vh)` — the oracle's
                   undistort_points under the identity rotation (x / 1: the ray itself; (-1e6, -1e6) where the inverse is None) — and v1 .. v3 (:69-77)
  delta            :58-68 through M = f32(K * f64(R)): ((m0 x) + m1 y) + m2 per row, two divides, `/ (vw, vh) - pos`
  solve_given      solve_ypr_given :124-192, 30 steps; returns q (the function's `rotation`: every caller inverts its result again, and the conjugate is exact)
  estimate         solve_ypr_ransac :194-238 with THE DRAWS AS DATA: the reference draws from an unseeded `rand::rng()` and has no reproducible output

The reference tree holds neither nalgebra's nor rand's source.  `UnitQuaternion::to_rotation_matrix`, `from_euler_angles` (quaternion and matrix), the Hamilton
product and `LU` (partial pivoting: the first largest |a| of the column, inv = 1 / pivot, multipliers a * inv, updates a + (-m) u, the row swaps, the unit lower
triangle forward and the upper triangle backward column by column, zeros when a pivot is exactly 0) are RESTATED here from the crates' documented forms: this
file is pinned only by itself and by what it is for — tests/test_pose_statement.py holds it to recovering a planted rotation before anything is compared with it.

Arithmetic: float32 numpy arrays, one rounding per written operator, batched over rounds (elementwise operations round like scalar ones); sums are sequential
folds from 0.0f in the order of the point list (np.add.accumulate); K * R in float64.  sinf / cosf / atanf are the host build of gyroflow_amd/csrc/gfw_math.h,
which tests/test_math_host.py pins to libm on all 2^32 inputs — not numpy's.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
PI32 = f32(np.pi)
EPS = (f32(0.001) * PI32) / f32(180.0)                                              # :9
STEPS = 30                                                                            # (15.0 / ALPHA).ceil()
NONE_PT = f32(-1000000.0)                                                             # cpu_undistort.rs:855

_MATH_SRC = r"""
#include "%s/gyroflow_amd/csrc/gfw_math.h"
void pm_sinf(const float *x, float *y, long n) { for (long i = 0; i < n; ++i) y[i] = gfw_sinf(x[i]); }
void pm_cosf(const float *x, float *y, long n) { for (long i = 0; i < n; ++i) y[i] = gfw_cosf(x[i]); }
void pm_atanf(const float *x, float *y, long n) { for (long i = 0; i < n; ++i) y[i] = gfw_atanf(x[i]); }
"""
_math = None


def _mathlib():
    global _math
    if _math is None:
        src = _MATH_SRC % ROOT
        hdr = open(os.path.join(ROOT, "gyroflow_amd", "csrc", "gfw_math.h")).read()
        d = os.path.join(ROOT, "build", "posestmt")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "math_%s.so" % hashlib.sha256((src + hdr).encode()).hexdigest()[:16])
        if not os.path.exists(so):
            c, tmp = "%s.%d.c" % (so, os.getpid()), "%s.%d.tmp" % (so, os.getpid())
            open(c, "w").write(src)
            subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", c, "-o", tmp, "-lm"])
            os.remove(c)
            os.replace(tmp, so)
        _math = C.CDLL(so)
    return _math


def _fn(name, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    getattr(_mathlib(), name)(C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), C.c_long(x.size))
    return y


def sinf(x):
    return _fn("pm_sinf", x)


def cosf(x):
    return _fn("pm_cosf", x)


def atanf(x):
    return _fn("pm_atanf", x)


class Camera:
    """What a call shares: the lens (a tests/_zoomstmt.Clip supplies KernelParams and the lens ids), the video and optical-flow sizes, K."""

    def __init__(self, clip, flow_size, num_iters=200, num_samples=1000, inlier_angle=0.05):
        self.clip, self.video, self.flow = clip, tuple(clip.size), tuple(flow_size)
        self.kp = clip.kernel_params()
        self.kp.lens_correction_amount = 1.0                                          # undistort_points(.., 1.0, 1.0, ..) (:65)
        self.K = np.array([[float(self.kp.f[0]), 0.0, float(self.kp.c[0])], [0.0, float(self.kp.f[1]), float(self.kp.c[1])], [0.0, 0.0, 1.0]])
        self.num_iters, self.num_samples, self.inlier_angle = int(num_iters), int(num_samples), f32(inlier_angle)


# ------------------------------------------------------------------------------------------------ the rotation algebra, batched: arrays [B] or [B][..]
def qmatrix(q):
    """UnitQuaternion::to_rotation_matrix: q [B][4] (w, i, j, k) -> R [B][9] row-major"""
    w, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two = f32(2.0)
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    ij, wk, wj, ik, jk, wi = (i * j) * two, (w * k) * two, (w * j) * two, (i * k) * two, (j * k) * two, (w * i) * two
    return np.stack([((ww + ii) - jj) - kk, ij - wk, wj + ik, wk + ij, ((ww - ii) + jj) - kk, jk - wi, ik - wj, wi + jk, ((ww - ii) - jj) + kk], axis=1)


def kr(K, R):
    """M = f32(K * f64(R)): ((k_i0 r_0j) + k_i1 r_1j) + k_i2 r_2j in float64"""
    Rd = R.astype(np.float64)
    cols = []
    for i in range(3):
        for j in range(3):
            cols.append(((K[i, 0] * Rd[:, j]) + K[i, 1] * Rd[:, 3 + j]) + K[i, 2] * Rd[:, 6 + j])
    return np.stack(cols, axis=1).astype(np.float32)


def euler_matrix(roll, pitch, yaw):
    """Rotation3::from_euler_angles -> [1][9]"""
    a = np.array([roll, pitch, yaw], dtype=np.float32)
    (sr, sp, sy), (cr, cp, cy) = sinf(a), cosf(a)
    return np.array([[cy * cp, ((cy * sp) * sr) - (sy * cr), ((cy * sp) * cr) + (sy * sr),
                      sy * cp, ((sy * sp) * sr) + (cy * cr), ((sy * sp) * cr) - (cy * sr),
                      -sp, cp * sr, cp * cr]], dtype=np.float32)


def euler_quat(roll, pitch, yaw):
    """UnitQuaternion::from_euler_angles of arrays [B] -> [B][4]: the half angles through sin_cos"""
    half = f32(0.5)
    hr, hp, hy = roll * half, pitch * half, yaw * half
    sr, cr, sp, cp, sy, cy = sinf(hr), cosf(hr), sinf(hp), cosf(hp), sinf(hy), cosf(hy)
    return np.stack([((cr * cp) * cy) + ((sr * sp) * sy), ((sr * cp) * cy) - ((cr * sp) * sy),
                     ((cr * sp) * cy) + ((sr * cp) * sy), ((cr * cp) * sy) - ((sr * sp) * cy)], axis=1)


def qmul(a, b):
    """the Hamilton product, [B][4]"""
    aw, ai, aj, ak = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bw, bi, bj, bk = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([(((aw * bw) - (ai * bi)) - (aj * bj)) - (ak * bk),
                     (((aw * bi) + (ai * bw)) + (aj * bk)) - (ak * bj),
                     (((aw * bj) - (ai * bk)) + (aj * bw)) + (ak * bi),
                     (((aw * bk) + (ai * bj)) - (aj * bi)) + (ak * bw)], axis=1)


def _swap(c, x, y):
    return np.where(c, y, x), np.where(c, x, y)


def lu(A):
    """LU with partial pivoting of A [B][9] row-major -> the factors (a dict of [B] arrays)"""
    with np.errstate(all="ignore"):
        a00, a01, a02, a10, a11, a12, a20, a21, a22 = [A[:, i].astype(np.float32) for i in range(9)]
        big, p0 = np.abs(a00), np.zeros(len(A), dtype=np.int32)
        c = np.abs(a10) > big
        big, p0 = np.where(c, np.abs(a10), big), np.where(c, 1, p0)
        p0 = np.where(np.abs(a20) > big, 2, p0)
        c = p0 == 1
        (a00, a10), (a01, a11), (a02, a12) = _swap(c, a00, a10), _swap(c, a01, a11), _swap(c, a02, a12)
        c = p0 == 2
        (a00, a20), (a01, a21), (a02, a22) = _swap(c, a00, a20), _swap(c, a01, a21), _swap(c, a02, a22)
        inv0 = f32(1.0) / a00
        m1, m2 = a10 * inv0, a20 * inv0
        a11, a12 = a11 + ((-m1) * a01), a12 + ((-m1) * a02)
        a21, a22 = a21 + ((-m2) * a01), a22 + ((-m2) * a02)
        p1 = np.abs(a21) > np.abs(a11)
        (a11, a21), (a12, a22), (m1, m2) = _swap(p1, a11, a21), _swap(p1, a12, a22), _swap(p1, m1, m2)
        inv1 = f32(1.0) / a11
        m21 = a21 * inv1
        a22 = a22 + ((-m21) * a12)
    return dict(u00=a00, u01=a01, u02=a02, u11=a11, u12=a12, u22=a22, l10=m1, l20=m2, l21=m21, p0=p0, p1=p1,
                singular=(a00 == 0.0) | (a11 == 0.0) | (a22 == 0.0))


def lu_solve(L, b0, b1, b2):
    """`decomp.solve(&b).unwrap_or_default()` -> x [B][3]"""
    with np.errstate(all="ignore"):
        b0, b1 = _swap(L["p0"] == 1, b0, b1)
        b0, b2 = _swap(L["p0"] == 2, b0, b2)
        b1, b2 = _swap(L["p1"], b1, b2)
        b1, b2 = b1 + ((-b0) * L["l10"]), b2 + ((-b0) * L["l20"])
        b2 = b2 + ((-b1) * L["l21"])
        x2 = b2 / L["u22"]
        b0, b1 = b0 + ((-x2) * L["u02"]), b1 + ((-x2) * L["u12"])
        x1 = b1 / L["u11"]
        b0 = b0 + ((-x1) * L["u01"])
        x0 = b0 / L["u00"]
    z = f32(0.0)
    return np.stack([np.where(L["singular"], z, x0), np.where(L["singular"], z, x1), np.where(L["singular"], z, x2)], axis=1).astype(np.float32)


def fold(x):
    """`sum::<f32>()` over axis 1 of [B][P]: the sequential fold from 0.0f in list order"""
    x = np.concatenate([np.zeros((x.shape[0], 1), dtype=np.float32), x.astype(np.float32)], axis=1)
    return np.add.accumulate(x, axis=1, dtype=np.float32)[:, -1]


def dot(a, b):
    return (a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])


# ------------------------------------------------------------------------------------------------ the camera
def delta(cam, M, ray, pos):
    """Camera::delta: M [B][9], ray [B][P][3] (x, y, ok), pos [B][P][2] -> [B][P][2]"""
    m = M[:, None, :]
    x, y = ray[..., 0], ray[..., 1]
    with np.errstate(all="ignore"):
        pr0 = ((m[..., 0] * x) + m[..., 1] * y) + m[..., 2]
        pr1 = ((m[..., 3] * x) + m[..., 4] * y) + m[..., 5]
        pr2 = ((m[..., 6] * x) + m[..., 7] * y) + m[..., 8]
        ok = ray[..., 2] != 0.0
        ptx, pty = np.where(ok, pr0 / pr2, NONE_PT), np.where(ok, pr1 / pr2, NONE_PT)
        return np.stack([(ptx / f32(cam.video[0])) - pos[..., 0], (pty / f32(cam.video[1])) - pos[..., 1]], axis=-1).astype(np.float32)


def prepare(cam, points_a, points_b):
    """-> dict(pos [n][2], motion [n][2], ray [n][3], v [n][3][2]) of one pair"""
    a, b = np.asarray(points_a, dtype=np.float32).reshape(-1, 2), np.asarray(points_b, dtype=np.float32).reshape(-1, 2)
    size = np.array(cam.flow, dtype=np.float32)
    pos, motion = a / size, (b - a) / size                                            # :28-30
    n = len(a)
    ray = np.zeros((n, 3), dtype=np.float32)
    if n:
        px = (pos * np.array(cam.video, dtype=np.float32)).astype(np.float32)         # :65
        r = O.undistort_points(cam.kp, cam.clip.model, cam.clip.digital, np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1]], dtype=np.float32), points=px)
        none = (r[:, 0] == NONE_PT) & (r[:, 1] == NONE_PT)
        ray[:, :2], ray[:, 2] = r, np.where(none, 0.0, 1.0)
    v = np.zeros((n, 3, 2), dtype=np.float32)
    z = f32(0.0)
    for k, e in enumerate((euler_matrix(z, EPS, z), euler_matrix(EPS, z, z), euler_matrix(z, z, -EPS))):      # roll, pitch, yaw (:69-77)
        v[:, k] = delta(cam, kr(cam.K, e), ray[None], pos[None])[0]
    return dict(pos=pos, motion=motion, ray=ray, v=v)


def solve_given(cam, P, idx):
    """solve_ypr_given over the points idx [B][p] of a prepared pair (B independent point lists of one length) -> q [B][4]"""
    idx = np.asarray(idx, dtype=np.int64)
    B = idx.shape[0]
    pos, motion, ray, v = P["pos"][idx], P["motion"][idx], P["ray"][idx], P["v"][idx]      # [B][p][..]
    A = np.stack([fold(dot(v[:, :, c], v[:, :, r])) for r in range(3) for c in range(3)], axis=1)
    L = lu(A)
    q = np.tile(np.array([[1, 0, 0, 0]], dtype=np.float32), (B, 1))
    z = np.zeros(B, dtype=np.float32)
    for step in range(STEPS):
        alpha = f32(1.0) if step == STEPS - 1 else f32(0.5)
        v0 = motion - delta(cam, kr(cam.K, qmatrix(q)), ray, pos)
        with np.errstate(all="ignore"):
            b = [fold(dot(v[:, :, r], v0)) for r in range(3)]
            model = (lu_solve(L, b[0], b[1], b[2]) * EPS) * alpha
            roll, pitch, yaw = euler_quat(z, model[:, 0], z), euler_quat(model[:, 1], z, z), euler_quat(z, z, -model[:, 2])
            q = qmul(q, qmul(qmul(pitch, roll), yaw))
    return q


def inliers(cam, P, q, lists):
    """the inlier test (:213-224) of the points lists [B][m] under the fits q [B][4] -> bool [B][m]"""
    lists = np.asarray(lists, dtype=np.int64)
    pos, motion, ray = P["pos"][lists], P["motion"][lists], P["ray"][lists]
    d = delta(cam, kr(cam.K, qmatrix(q)), ray, pos)
    sample, vec = pos + d, motion - d
    K = cam.K.astype(np.float32)
    target = cam.inlier_angle * (PI32 / f32(180.0))
    with np.errstate(all="ignore"):
        ax, ay = atanf((sample[..., 0] - K[0, 2]) / K[0, 0]), atanf((sample[..., 1] - K[1, 2]) / K[1, 1])      # point_angle (:46-57): as written
        ex, ey = vec[..., 0] * cosf(ax).reshape(ax.shape), vec[..., 1] * cosf(ay).reshape(ay.shape)
        return ((ex * ex) + (ey * ey)) <= (target * target)


def estimate_pair(cam, points_a, points_b, triples, samples=None):
    """One pair -> dict(quat [4] f32, rotation [3][3] f64, best (inliers, round), round_inliers [num_iters], round_fits [num_iters][4], inlier_idx [..])"""
    P = prepare(cam, points_a, points_b)
    n, iters = len(P["pos"]), cam.num_iters
    ident = np.array([1, 0, 0, 0], dtype=np.float32)
    counts, fits = np.zeros(iters, dtype=np.int32), np.tile(ident, (iters, 1))
    q, best, keep = ident, (0, 0 if iters else -1), np.zeros(0, dtype=np.int64)
    if n >= 3 and iters:
        m = min(n, cam.num_samples)
        lists = np.tile(np.arange(n), (iters, 1)) if samples is None else np.asarray(samples, dtype=np.int64).reshape(iters, m)
        assert samples is not None or n <= cam.num_samples
        fits = solve_given(cam, P, np.asarray(triples, dtype=np.int64).reshape(iters, 3))
        inl = inliers(cam, P, fits, lists)
        counts = inl.sum(axis=1).astype(np.int32)
        rnd = int(np.argmax(counts))                                                  # the first of the maximal rounds: `if inliers.len() > best_inliers.len()`
        best, keep = (int(counts[rnd]), rnd), lists[rnd][inl[rnd]]
        if best[0] >= 3:
            q = solve_given(cam, P, keep[None])[0]
    rot = qmatrix(q[None])[0].astype(np.float64).reshape(3, 3)
    return dict(quat=q.astype(np.float32), rotation=rot, best=best, round_inliers=counts, round_fits=fits.astype(np.float32), inlier_idx=keep)


def estimate(cam, pairs, triples, samples=None):
    """gfw_pose_almeida's outputs for pairs [(points_a, points_b)] -> (quats [n][4], rotations [n][3][3], best [n][2], round_inliers [n][iters], round_fits [n][iters][4])"""
    out = [estimate_pair(cam, a, b, triples[p], None if samples is None else samples[p]) for p, (a, b) in enumerate(pairs)]
    n, iters = len(pairs), cam.num_iters
    stack = lambda key, shape, dt: np.array([o[key] for o in out], dtype=dt).reshape(shape)
    return (stack("quat", (n, 4), np.float32), stack("rotation", (n, 3, 3), np.float64), stack("best", (n, 2), np.int32),
            stack("round_inliers", (n, iters), np.int32), stack("round_fits", (n, iters, 4), np.float32))
