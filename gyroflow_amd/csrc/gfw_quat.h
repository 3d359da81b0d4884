// gfw_quat.h — the f64 quaternion-track device functions shared by the per-row matrix builder (gfw_matrices.hip), the zoom search
// (gfw_zoom.hip) and the sync search (gfw_sync.hip): GyroSource::quat_at_timestamp / offset_at_timestamp with the reference's rounding and clamping, nalgebra's slerp, and
// the rotation matrix of FrameTransform (image_rotation * R(quat)).
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_matrices.h"

namespace {

struct Q { double w, x, y, z; };
__device__ __forceinline__ Q qmul(const Q &a, const Q &b) {
    return Q{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
             a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
// nalgebra UnitQuaternion::slerp (Unit<Vector4>::try_slerp with the shorter-arc flip)
__device__ __forceinline__ Q slerp(const Q &a, Q b, double t) {
    double c = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;
    if (c < 0.0) { b = Q{-b.w, -b.x, -b.y, -b.z}; c = -c; }
    if (fabs(c) >= 1.0) return a;
    const double hang = acos(c);
    const double s = sqrt(1.0 - c * c);
    if (s == 0.0) return a;
    const double ta = sin((1.0 - t) * hang) / s, tb = sin(t * hang) / s;
    return Q{a.w * ta + b.w * tb, a.x * ta + b.x * tb, a.y * ta + b.y * tb, a.z * ta + b.z * tb};
}
// Rust `f64 as i64`: truncate toward zero, saturate, NaN -> 0
__device__ __forceinline__ int64_t f2i64(double v) {
    if (!(v == v)) return 0;
    if (v >= 9223372036854775807.0) return INT64_MAX;
    if (v <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)v;
}
// GyroSource::offset_at_timestamp (gyro_source/mod.rs:884-908): linear interpolation (and extrapolation) of the sync offsets
__device__ double offset_at(const int64_t *ts, const double *v, int n, double timestamp_ms) {
    if (n <= 0) return 0.0;
    if (n == 1) return v[0];
    const int64_t timestamp_us = f2i64(timestamp_ms * 1000.0);
    int64_t lookup = timestamp_us;
    if (lookup > ts[n - 1] - 1) lookup = ts[n - 1] - 1;           // .min(last_ts - 1)
    if (lookup < ts[0] + 1) lookup = ts[0] + 1;                   // .max(first_ts + 1)
    if (lookup < ts[0]) return 0.0;                               // range(..=lookup) empty
    int lo = 0, hi = n - 1;                                       // last index with ts[i] <= lookup
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ts[mid] <= lookup) lo = mid; else hi = mid - 1; }
    if (ts[lo] == lookup) return v[lo];
    if (lo + 1 >= n) return 0.0;                                  // range(lookup..) empty
    const double time_delta = (double)(ts[lo + 1] - ts[lo]);
    const double fract = (double)(timestamp_us - ts[lo]) / time_delta;
    return v[lo] + (v[lo + 1] - v[lo]) * fract;
}
// GyroSource::quat_at_timestamp (gyro_source/mod.rs:857-882) over a sorted (timestamp_us -> quaternion) track
__device__ Q quat_at(const GfwTracks &T, const int64_t *ts, const double *q, int n, double timestamp_ms) {
    if (n < 2 || !(T.duration_ms > 0.0)) return Q{1.0, 0.0, 0.0, 0.0};
    timestamp_ms -= offset_at(T.off_ts, T.off_ms, T.off_n, timestamp_ms);
    int64_t lookup = f2i64(round(timestamp_ms * 1000.0));
    if (lookup > ts[n - 1]) lookup = ts[n - 1];
    if (lookup < ts[0]) lookup = ts[0];
    int lo = 0, hi = n - 1;                     // last index with ts[i] <= lookup
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ts[mid] <= lookup) lo = mid; else hi = mid - 1; }
    const Q q1{q[lo * 4], q[lo * 4 + 1], q[lo * 4 + 2], q[lo * 4 + 3]};
    if (ts[lo] == lookup || lo + 1 >= n) return q1;
    const Q q2{q[lo * 4 + 4], q[lo * 4 + 5], q[lo * 4 + 6], q[lo * 4 + 7]};
    const double fract = (double)(lookup - ts[lo]) / (double)(ts[lo + 1] - ts[lo]);
    return slerp(q1, q2, fract);
}

// R(quat) of a (re-normalised) quaternion, then image_rotation * R (frame_transform.rs:258-259, :399-400); the sign flips are the caller's
__device__ __forceinline__ void quat_rotation(Q q, double video_rotation_deg, double r[3][3]) {
    const double nn = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    q = Q{q.w / nn, q.x / nn, q.y / nn, q.z / nn};
    r[0][0] = 1 - 2 * (q.y * q.y + q.z * q.z); r[0][1] = 2 * (q.x * q.y - q.z * q.w); r[0][2] = 2 * (q.x * q.z + q.y * q.w);
    r[1][0] = 2 * (q.x * q.y + q.z * q.w); r[1][1] = 1 - 2 * (q.x * q.x + q.z * q.z); r[1][2] = 2 * (q.y * q.z - q.x * q.w);
    r[2][0] = 2 * (q.x * q.z - q.y * q.w); r[2][1] = 2 * (q.y * q.z + q.x * q.w); r[2][2] = 1 - 2 * (q.x * q.x + q.y * q.y);
    if (video_rotation_deg != 0.0) {                                               // image_rotation * R
        const double a = video_rotation_deg * (3.14159265358979323846 / 180.0), ca = cos(a), sa = sin(a);
        for (int j = 0; j < 3; ++j) { const double r0 = r[0][j], r1 = r[1][j]; r[0][j] = ca * r0 - sa * r1; r[1][j] = sa * r0 + ca * r1; }
    }
}
// smoothed(ts) * org(ts)^-1 (frame_transform.rs:255-256, :389-390): the factor every row / point of a frame shares
__device__ __forceinline__ Q quat_prefix(const GfwTracks &T, double ts) {
    Q q1 = quat_at(T, T.org_ts, T.org_q, T.org_n, ts);
    const double n1 = q1.w * q1.w + q1.x * q1.x + q1.y * q1.y + q1.z * q1.z;
    q1 = Q{q1.w / n1, -q1.x / n1, -q1.y / n1, -q1.z / n1};                         // inverse()
    const Q sm = quat_at(T, T.sm_ts, T.sm_q, T.sm_n, ts);
    return qmul(sm, q1);
}

}  // namespace

// at_timestamp_for_points' rotation of one point, shared by the zoom search and the sync search (gfw_sync.hip) (frame_transform.rs:391-409): new_k * (image_rotation * R(prefix * org(quat_time))) with the four sign flips of
// :402-403 — always these, whatever framebuffer_inverted says — or new_k alone under suppress_rotation; -> f32, row-major
__device__ inline void gfw_zoom_rotation(const GfwTracks &T, const gfw_zoom_frame &F, const Q &pre, double quat_time, float out[9]) {
    double r[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    if (!F.suppress_rotation) {
        quat_rotation(qmul(pre, quat_at(T, T.org_ts, T.org_q, T.org_n, quat_time)), F.video_rotation_deg, r);
        r[0][1] *= -1.0; r[0][2] *= -1.0; r[1][0] *= -1.0; r[2][0] *= -1.0;
    }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
        out[i * 3 + j] = (float)(F.new_k[i * 3 + 0] * r[0][j] + F.new_k[i * 3 + 1] * r[1][j] + F.new_k[i * 3 + 2] * r[2][j]);
}
