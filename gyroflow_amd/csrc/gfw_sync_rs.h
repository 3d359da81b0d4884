// gfw_sync_rs.h — the rs-sync offset search of a clip's ranges on the device (gfw_sync_rs.hip): offset method 2 (find_offset/rs_sync.rs), the reference's default.
// The adapter is mirrored — per-point unit bearings and per-point timestamps in (:115-146), a delay and a cost out, the acceptance rule the mirrors' — but its
// solver, the `rs-sync` crate, is not part of the reference tree and is NOT reproduced: the search is stated operation by operation in tests/_rssyncstmt.py.
// Host and device: the f64 algebra below is one operation sequence (+ - * / sqrt, one rounding per written operator under -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_math.h"
#include "gfw_pose_essential.h"     // gfw_pe_bearing, gfw_pe_jacobi, gfw_pe_cross, GFW_PE_NONE

#define GFW_RS_LANES 256            // lanes of a prepare or pick workgroup (64 x 4); a cost workgroup is one wave
#define GFW_RS_PAIR_MAX 4096        // points of one pair: m_i of a (candidate, pair) lives in 24 B of LDS a point
#define GFW_RS_PAIRS_MAX 65535      // pairs ride on blockIdx.y
#define GFW_RS_RANGES_MAX 65535
#define GFW_RS_TRACK_MAX (1 << 24)  // samples of the quaternion track
#define GFW_RS_CANDIDATES_MAX (1 << 20)      // candidates of a range in one round
#define GFW_RS_ROUNDS_MAX 8
#define GFW_RS_LATER 17             // candidates of every round behind the first: pick + (i - 8) step / 8
#define GFW_RS_HYPOTHESES_MAX 64
#define GFW_RS_REFITS_MAX 16
#define GFW_RS_SWEEPS_MAX 32

struct GfwRsArgs {
    const int32_t *range_first;     // [n_ranges + 1] first pair of each range (device)
    const int32_t *pair_range;      // [n_pairs] the range of each pair (device)
    const int32_t *pair_first;      // [n_pairs + 1] first point of each pair (device)
    const int64_t *pair_ts;         // [n_pairs][2] timestamps_us of a pair's two frames (device)
    const float *points;            // [2][total][2]: every pair's points of the first frame, then of the second (device)
    const double *track_t;          // [n_track] seconds, ascending (device)
    const double *track_q;          // [n_track][4] (w, x, y, z) (device)
    const int32_t *cand_first;      // mode 0: [n_ranges + 1] first candidate of each range (device)
    const double *cand;             // mode 0: the caller's candidates, seconds (device)
    const int64_t *pc_first;        // mode 0: [n_pairs] first entry of each pair in pair_costs (device)
    double *prep;                   // [2][total][4] bearing and time of every point and side — the prepare stage's, work space
    double *pair_costs;             // one f64 per (pair, candidate): mode 0 at pc_first[pair] + c, else at pair * n_cand + c — work space
    double *cand_all;               // modes 1, 2: [n_ranges][total_cand] every round's candidates: the caller's round_candidates or work space
    double *sums_all;               // mode 0: the caller's costs (at cand_first[r] + c); else [n_ranges][total_cand]: the caller's round_costs or work space
    gfw_sync_result *results;       // modes 1, 2: [n_ranges]
    double initial, step, next_step, loss_scale, readout_s, flow_h;
    float vw, vh, fw, fh;           // video size, optical-flow image size as f32
    int32_t n_ranges, n_pairs, total, n_track;
    int32_t mode;                   // 0 the caller's candidates (gfw_sync_rs_costs); 1 round 0 of a search; 2 a later round
    int32_t n_cand, half, at, total_cand, last, refine;      // this round's candidates a range, h of round 0, the round's first entry in a range's row, the row, last round
    int32_t hypotheses, refits, sweeps, lds_points;           // .. points of the call's largest pair
};

// t clamped to the track's ends
GFW_HD double gfw_rs_clamp(const double *T, int n, double t) { return t < T[0] ? T[0] : (t > T[n - 1] ? T[n - 1] : t); }
// the segment of tc by bisection between lo and hi: the last i in lo .. hi - 1 with T[i] <= tc (lo where there is none)
GFW_HD int gfw_rs_segment(const double *T, int lo, int hi, double tc) {
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (T[mid] <= tc) lo = mid; else hi = mid;
    }
    return lo;
}
// the track at time t: clamped to its ends, the segment i with T[i] <= t (0 <= i <= n - 2), normalised linear interpolation, the shorter arc.  The bisection runs
// between wlo and whi: 0 and n - 1, or any window whose ends are the segments of two times around t (wlo = segment(t0), whi = segment(t1) + 1 for t0 <= t <= t1) —
// the segment found is the same, the last sample at or below t.
GFW_HD void gfw_rs_quat_in(const double *T, const double *Q, int n, int wlo, int whi, double t, double *q) {
    const double tc = gfw_rs_clamp(T, n, t);
    const int lo = gfw_rs_segment(T, wlo, whi, tc);
    const double f = (tc - T[lo]) / (T[lo + 1] - T[lo]);
    const double *a = Q + (size_t)lo * 4, *b = a + 4;
    const double dot = (((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])) + (a[3] * b[3]);
    const bool flip = dot < 0.0;
    #pragma unroll
    for (int k = 0; k < 4; ++k) { const double bk = flip ? -b[k] : b[k]; q[k] = a[k] + ((bk - a[k]) * f); }
    const double nrm = __builtin_sqrt((((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])) + (q[3] * q[3]));
    #pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] / nrm;
}
GFW_HD void gfw_rs_quat_at(const double *T, const double *Q, int n, double t, double *q) { gfw_rs_quat_in(T, Q, n, 0, n - 1, t, q); }
// the world bearing R(q) diag(1, -1, -1) p: the rotation by pi about X is set_quats' (rs_sync.rs:248-251)
GFW_HD void gfw_rs_to_world(const double *q, const double *p, double *o) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double p0 = p[0], p1 = -p[1], p2 = -p[2];
    const double r00 = 1.0 - (2.0 * ((y * y) + (z * z))), r01 = 2.0 * ((x * y) - (w * z)), r02 = 2.0 * ((x * z) + (w * y));
    const double r10 = 2.0 * ((x * y) + (w * z)), r11 = 1.0 - (2.0 * ((x * x) + (z * z))), r12 = 2.0 * ((y * z) - (w * x));
    const double r20 = 2.0 * ((x * z) - (w * y)), r21 = 2.0 * ((y * z) + (w * x)), r22 = 1.0 - (2.0 * ((x * x) + (y * y)));
    o[0] = ((r00 * p0) + (r01 * p1)) + (r02 * p2);
    o[1] = ((r10 * p0) + (r11 * p1)) + (r12 * p2);
    o[2] = ((r20 * p0) + (r21 * p1)) + (r22 * p2);
}
// m = ra x rb of one point at delay d; pa, pb: (bearing, time) of its two sides; wlo, whi: the bisection's window (0, n - 1: the whole track)
GFW_HD void gfw_rs_moment_vector(const double *T, const double *Q, int n, int wlo, int whi, const double *pa, const double *pb, double d, double *m) {
    double q[4], ra[3], rb[3];
    gfw_rs_quat_in(T, Q, n, wlo, whi, pa[3] + d, q);
    gfw_rs_to_world(q, pa, ra);
    gfw_rs_quat_in(T, Q, n, wlo, whi, pb[3] + d, q);
    gfw_rs_to_world(q, pb, rb);
    gfw_pe_cross(ra, rb, m);
}
// the eigenvector of the smallest eigenvalue of the symmetric G (00, 01, 02, 11, 12, 22; destroyed), the first of equal ones
GFW_HD void gfw_rs_smallest(double *G, int sweeps, double *t) {
    double V[9];
    gfw_pe_jacobi<3, 0>(G, V, nullptr, 0, sweeps);
    double low = G[0];
    t[0] = V[0]; t[1] = V[3]; t[2] = V[6];
    const bool c1 = G[3] < low;
    low = c1 ? G[3] : low;
    t[0] = c1 ? V[1] : t[0]; t[1] = c1 ? V[4] : t[1]; t[2] = c1 ? V[7] : t[2];
    const bool c2 = G[5] < low;
    t[0] = c2 ? V[2] : t[0]; t[1] = c2 ? V[5] : t[1]; t[2] = c2 ? V[8] : t[2];
}
// x^2 of a point under the direction t, x = k (m . t)
GFW_HD double gfw_rs_residual2(double k, double m0, double m1, double m2, const double *t) {
    const double x = k * (((m0 * t[0]) + (m1 * t[1])) + (m2 * t[2]));
    return x * x;
}

// the prepare stage of 2 x `total` lanes; the cost stage, a one-wave workgroup per (candidate, pair); the pick stage, a workgroup per range.  Zero-sized launches are skipped.
hipError_t gfw_launch_rs_prepare(const gfw_kernel_params &P, const GfwCommon &C, const GfwRsArgs &A, hipStream_t s);
hipError_t gfw_launch_rs_costs(const GfwRsArgs &A, int max_candidates, hipStream_t s);
hipError_t gfw_launch_rs_pick(const GfwRsArgs &A, hipStream_t s);
