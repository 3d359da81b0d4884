// gfw_pose_math.h — host and device: the f32 rotation algebra of the Almeida estimator (almeida.rs:124-192) as one operation sequence — nalgebra's
// `UnitQuaternion::to_rotation_matrix`, `from_euler_angles` (quaternion and matrix), the Hamilton product and the 3 x 3 `LU` with partial pivoting, restated from
// the crate's documented forms (its source is not part of the reference tree: tests/_posestmt.py is the statement both sides are held to).  One rounding per written
// operator (-ffp-contract=off); sines and cosines are gfw_math.h's.  No indexing by a run-time value: everything stays in registers.
#pragma once
#include "gfw_math.h"

#define GFW_POSE_EPS ((0.001f * 3.14159265358979323846f) / 180.0f)      // `0.001 * PI / 180.0` (:9)

struct GfwQ4 { float w, i, j, k; };

// UnitQuaternion::to_rotation_matrix -> R row-major
GFW_HD void gfw_pose_qmatrix(const GfwQ4 q, float *R) {
    const float ww = q.w * q.w, ii = q.i * q.i, jj = q.j * q.j, kk = q.k * q.k;
    const float ij = (q.i * q.j) * 2.0f, wk = (q.w * q.k) * 2.0f, wj = (q.w * q.j) * 2.0f;
    const float ik = (q.i * q.k) * 2.0f, jk = (q.j * q.k) * 2.0f, wi = (q.w * q.i) * 2.0f;
    R[0] = ((ww + ii) - jj) - kk; R[1] = ij - wk;               R[2] = wj + ik;
    R[3] = wk + ij;               R[4] = ((ww - ii) + jj) - kk; R[5] = jk - wi;
    R[6] = ik - wj;               R[7] = wi + jk;               R[8] = ((ww - ii) - jj) + kk;
}
// M = f32(K * f64(R)): `camera_matrix * na::convert(rot)` of undistort_points, the f64 product ((k_i0 r_0j) + k_i1 r_1j) + k_i2 r_2j
GFW_HD void gfw_pose_kr(const double *K, const float *R, float *M) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[i * 3 + j] = (float)(((K[i * 3] * (double)R[j]) + K[i * 3 + 1] * (double)R[3 + j]) + K[i * 3 + 2] * (double)R[6 + j]);
}
// Rotation3::from_euler_angles(roll, pitch, yaw) -> R row-major
GFW_HD void gfw_pose_euler_matrix(float roll, float pitch, float yaw, float *R) {
    const float sr = gfw_sinf(roll), cr = gfw_cosf(roll), sp = gfw_sinf(pitch), cp = gfw_cosf(pitch), sy = gfw_sinf(yaw), cy = gfw_cosf(yaw);
    R[0] = cy * cp; R[1] = ((cy * sp) * sr) - (sy * cr); R[2] = ((cy * sp) * cr) + (sy * sr);
    R[3] = sy * cp; R[4] = ((sy * sp) * sr) + (cy * cr); R[5] = ((sy * sp) * cr) - (cy * sr);
    R[6] = -sp;     R[7] = cp * sr;                      R[8] = cp * cr;
}
// UnitQuaternion::from_euler_angles(roll, pitch, yaw): the half angles through sin_cos
GFW_HD GfwQ4 gfw_pose_euler_quat(float roll, float pitch, float yaw) {
    const float hr = roll * 0.5f, hp = pitch * 0.5f, hy = yaw * 0.5f;
    const float sr = gfw_sinf(hr), cr = gfw_cosf(hr), sp = gfw_sinf(hp), cp = gfw_cosf(hp), sy = gfw_sinf(hy), cy = gfw_cosf(hy);
    GfwQ4 q;
    q.w = ((cr * cp) * cy) + ((sr * sp) * sy);
    q.i = ((sr * cp) * cy) - ((cr * sp) * sy);
    q.j = ((cr * sp) * cy) + ((sr * cp) * sy);
    q.k = ((cr * cp) * sy) - ((sr * sp) * cy);
    return q;
}
// the Hamilton product a * b
GFW_HD GfwQ4 gfw_pose_qmul(const GfwQ4 a, const GfwQ4 b) {
    GfwQ4 q;
    q.w = (((a.w * b.w) - (a.i * b.i)) - (a.j * b.j)) - (a.k * b.k);
    q.i = (((a.w * b.i) + (a.i * b.w)) + (a.j * b.k)) - (a.k * b.j);
    q.j = (((a.w * b.j) - (a.i * b.k)) + (a.j * b.w)) + (a.k * b.i);
    q.k = (((a.w * b.k) + (a.i * b.j)) - (a.j * b.i)) + (a.k * b.w);
    return q;
}

// LU of a 3 x 3 with partial pivoting: the pivot of a column is its first largest |a|; inv = 1 / pivot, multipliers a * inv, updates a_ij + (-m_i) u_j
struct GfwLu3 { float u00, u01, u02, u11, u12, u22, l10, l20, l21; int p0, p1, singular; };     // p0: the row swapped with row 0 (0, 1, 2); p1: rows 1 and 2 swapped
GFW_HD GfwLu3 gfw_pose_lu(const float *A) {
    float a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[3], a11 = A[4], a12 = A[5], a20 = A[6], a21 = A[7], a22 = A[8], t;
    GfwLu3 L;
    L.p0 = 0;
    float big = gfw_fabsf(a00);
    if (gfw_fabsf(a10) > big) { big = gfw_fabsf(a10); L.p0 = 1; }
    if (gfw_fabsf(a20) > big) L.p0 = 2;
    if (L.p0 == 1) { t = a00; a00 = a10; a10 = t; t = a01; a01 = a11; a11 = t; t = a02; a02 = a12; a12 = t; }
    if (L.p0 == 2) { t = a00; a00 = a20; a20 = t; t = a01; a01 = a21; a21 = t; t = a02; a02 = a22; a22 = t; }
    const float inv0 = 1.0f / a00;
    float m1 = a10 * inv0, m2 = a20 * inv0;
    a11 = a11 + ((-m1) * a01); a12 = a12 + ((-m1) * a02);
    a21 = a21 + ((-m2) * a01); a22 = a22 + ((-m2) * a02);
    L.p1 = gfw_fabsf(a21) > gfw_fabsf(a11) ? 1 : 0;
    if (L.p1) { t = a11; a11 = a21; a21 = t; t = a12; a12 = a22; a22 = t; t = m1; m1 = m2; m2 = t; }
    const float inv1 = 1.0f / a11;
    const float m21 = a21 * inv1;
    a22 = a22 + ((-m21) * a12);
    L.u00 = a00; L.u01 = a01; L.u02 = a02; L.u11 = a11; L.u12 = a12; L.u22 = a22; L.l10 = m1; L.l20 = m2; L.l21 = m21;
    L.singular = (a00 == 0.0f || a11 == 0.0f || a22 == 0.0f) ? 1 : 0;
    return L;
}
// `decomp.solve(&b).unwrap_or_default()`: the row swaps, the unit lower triangle forward and the upper triangle backward, column by column
// (b_k = b_k + (-x_i) a_ki); zeros when a pivot is exactly 0
GFW_HD void gfw_pose_lu_solve(const GfwLu3 &L, float b0, float b1, float b2, float &x0, float &x1, float &x2) {
    float t;
    if (L.p0 == 1) { t = b0; b0 = b1; b1 = t; }
    if (L.p0 == 2) { t = b0; b0 = b2; b2 = t; }
    if (L.p1) { t = b1; b1 = b2; b2 = t; }
    b1 = b1 + ((-b0) * L.l10); b2 = b2 + ((-b0) * L.l20);
    b2 = b2 + ((-b1) * L.l21);
    x2 = b2 / L.u22;
    b0 = b0 + ((-x2) * L.u02); b1 = b1 + ((-x2) * L.u12);
    x1 = b1 / L.u11;
    b0 = b0 + ((-x1) * L.u01);
    x0 = b0 / L.u00;
    if (L.singular) { x0 = 0.0f; x1 = 0.0f; x2 = 0.0f; }
}
// One step's update (:175-187): q * ((pitch * roll) * yaw) of the scaled model, no renormalisation
GFW_HD GfwQ4 gfw_pose_update(const GfwQ4 q, const GfwLu3 &L, float b0, float b1, float b2, float alpha) {
    float x, y, z;
    gfw_pose_lu_solve(L, b0, b1, b2, x, y, z);
    x = (x * GFW_POSE_EPS) * alpha; y = (y * GFW_POSE_EPS) * alpha; z = (z * GFW_POSE_EPS) * alpha;
    const GfwQ4 roll = gfw_pose_euler_quat(0.0f, x, 0.0f), pitch = gfw_pose_euler_quat(y, 0.0f, 0.0f), yaw = gfw_pose_euler_quat(0.0f, 0.0f, -z);
    return gfw_pose_qmul(q, gfw_pose_qmul(gfw_pose_qmul(pitch, roll), yaw));
}
// The matrices f32(K * E) of the three derivative rotations: E(0, EPS, 0), E(EPS, 0, 0), E(0, 0, -EPS) (roll, pitch, yaw: :69-77) -> [3][9]
GFW_HD void gfw_pose_eps_matrices(const double *K, float *M27) {
    float R[9];
    gfw_pose_euler_matrix(0.0f, GFW_POSE_EPS, 0.0f, R); gfw_pose_kr(K, R, M27);
    gfw_pose_euler_matrix(GFW_POSE_EPS, 0.0f, 0.0f, R); gfw_pose_kr(K, R, M27 + 9);
    gfw_pose_euler_matrix(0.0f, 0.0f, -GFW_POSE_EPS, R); gfw_pose_kr(K, R, M27 + 18);
}
