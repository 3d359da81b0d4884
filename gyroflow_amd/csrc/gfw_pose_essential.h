// gfw_pose_essential.h — essential-matrix pose estimation of a clip's frame pairs on the device (gfw_pose_essential.hip): what the reference's pose methods 0
// (`PoseFindEssentialMat`) and 2 (`PoseEightPoint`, estimate_pose/mod.rs:27-36) are for — an essential matrix fitted to the undistorted bearings of a pair's matched
// points, its rotation part returned.  Their solvers (OpenCV's findEssentialMat / recoverPose, the arrsac and eight-point crates) are not part of the reference tree
// and are NOT reproduced: this is the published eight-point scheme inside a RANSAC loop, stated operation by operation in tests/_posessstmt.py, the draws an input.
// Host and device: the f64 algebra below is one operation sequence (+ - * / sqrt, one rounding per written operator under -ffp-contract=off), with every array
// register index a compile-time constant after unrolling, so what a lane keeps of its matrices in registers stays there.
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_math.h"

#define GFW_PE_LANES 256            // lanes of a workgroup (64 x 4); a fit workgroup is 256 rounds of a pair (one-wave workgroups ran 3.3 x slower)
#define GFW_PE_PAIR_MAX 4096        // points of one pair: the best round's inliers are packed as 16-bit indices in 8 KB of LDS
#define GFW_PE_PAIRS_MAX 65535      // pairs ride on blockIdx.y
#define GFW_PE_ROUNDS_MAX 1024      // RANSAC rounds of a pair
#define GFW_PE_MIN_POINTS 8         // points of a fit
#define GFW_PE_SWEEPS9 10           // cyclic Jacobi sweeps of the 9 x 9 moment matrix (every matrix of the test plants has converged after 8: DESIGN.md 3.2m)
#define GFW_PE_SWEEPS3 8            // .. of the 3 x 3 E^T E
#define GFW_PE_BIG 1e150            // |theta| from which theta * theta would overflow: t = 1 / (2 theta)
#define GFW_PE_NONE (-1000000.0f)   // a point without a lens inverse (cpu_undistort.rs:855)

struct GfwPoseEssArgs {
    const int32_t *pair_first;      // [n_pairs + 1] first point of each pair (device)
    const float *points;            // [2][total][2]: every pair's points of the first frame, then of the second (device)
    const int32_t *octets;          // [n_pairs][num_iters][8] indices into the pair (device)
    float4 *und;                    // [total] the undistorted (x1, y1, x2, y2)                — the prepare stage's, work space
    double *fits;                   // [n_pairs][num_iters][9] E of every round: the caller's round_fits or work space
    int32_t *counts;                // [n_pairs][num_iters] inliers of every round: the caller's round_inliers or work space
    float *quats;                   // [n_pairs][4]
    double *rotations;              // [n_pairs][9]
    double *essential;              // [n_pairs][9]
    int32_t *best;                  // [n_pairs][4] inliers, round, front, found
    double threshold;               // squared Sampson distance of an inlier, normalised units
    float vw, vh, fw, fh;           // video size, optical-flow image size as f32
    int32_t n_pairs, total, num_iters, min_front;
};

// index of (i, j) in the row-major upper triangle of a symmetric N x N
#define GFW_PE_TRI(N, i, j) ((i) <= (j) ? (i) * (N) - (i) * ((i) - 1) / 2 + ((j) - (i)) : (j) * (N) - (j) * ((j) - 1) / 2 + ((i) - (j)))

// the unit bearing of the normalised point (x, y, 1) (eight_point.rs:29-34)
GFW_HD void gfw_pe_bearing(double x, double y, double *b) {
    const double n = __builtin_sqrt(((x * x) + (y * y)) + 1.0);
    b[0] = x / n; b[1] = y / n; b[2] = 1.0 / n;
}
// kron(b2, b1) of one point's undistorted (x1, y1, x2, y2)
GFW_HD void gfw_pe_kron(const float4 u, double *a) {
    double b1[3], b2[3];
    gfw_pe_bearing((double)u.x, (double)u.y, b1);
    gfw_pe_bearing((double)u.z, (double)u.w, b2);
    #pragma unroll
    for (int i = 0; i < 3; ++i) {
        #pragma unroll
        for (int j = 0; j < 3; ++j) a[i * 3 + j] = b2[i] * b1[j];
    }
}

// One cyclic Jacobi sweep of the symmetric A (upper triangle, N (N + 1) / 2) with the eigenvectors accumulated in the columns of V (N x N row-major): (p, q) in
// row order, a rotation skipped where the off-diagonal is exactly 0.  The first N - NL rows of V are the array `V` (registers); the last NL rows live behind `VL`,
// entry (k, j) at VL[((k - (N - NL)) * N + j) * stride] — a lane's column of an LDS array on the device, so that triangle, eigenvectors and temporaries stay under
// 256 registers.  Where a value is kept does not change it: the operation sequence is one.
template <int N, int NL>
GFW_HD void gfw_pe_sweep(double *A, double *V, double *VL, int stride) {
    #pragma unroll
    for (int p = 0; p < N - 1; ++p) {
        #pragma unroll
        for (int q = p + 1; q < N; ++q) {
            const double apq = A[GFW_PE_TRI(N, p, q)];
            if (apq != 0.0) {
                const double theta = (A[GFW_PE_TRI(N, q, q)] - A[GFW_PE_TRI(N, p, p)]) / (apq + apq);
                const double mag = __builtin_fabs(theta);
                const bool big = mag >= GFW_PE_BIG;
                const double num = big ? 1.0 : (theta >= 0.0 ? 1.0 : -1.0);
                const double den = big ? theta + theta : mag + __builtin_sqrt((theta * theta) + 1.0);
                const double t = num / den;
                const double c = 1.0 / __builtin_sqrt((t * t) + 1.0);
                const double s = t * c;
                #pragma unroll
                for (int k = 0; k < N; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[GFW_PE_TRI(N, k, p)], akq = A[GFW_PE_TRI(N, k, q)];
                        A[GFW_PE_TRI(N, k, p)] = (c * akp) - (s * akq);
                        A[GFW_PE_TRI(N, k, q)] = (s * akp) + (c * akq);
                    }
                }
                A[GFW_PE_TRI(N, p, p)] = A[GFW_PE_TRI(N, p, p)] - (t * apq);
                A[GFW_PE_TRI(N, q, q)] = A[GFW_PE_TRI(N, q, q)] + (t * apq);
                A[GFW_PE_TRI(N, p, q)] = 0.0;
                #pragma unroll
                for (int k = 0; k < N - NL; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = (c * vkp) - (s * vkq);
                    V[k * N + q] = (s * vkp) + (c * vkq);
                }
                #pragma unroll
                for (int k = 0; k < NL; ++k) {
                    double *vp = VL + (size_t)(k * N + p) * stride, *vq = VL + (size_t)(k * N + q) * stride;
                    const double vkp = *vp, vkq = *vq;
                    *vp = (c * vkp) - (s * vkq);
                    *vq = (s * vkp) + (c * vkq);
                }
            }
        }
    }
}
template <int N, int NL>
GFW_HD void gfw_pe_jacobi(double *A, double *V, double *VL, int stride, int sweeps) {
    #pragma unroll
    for (int i = 0; i < (N - NL) * N; ++i) V[i] = (i / N == i % N) ? 1.0 : 0.0;
    #pragma unroll
    for (int i = 0; i < NL * N; ++i) VL[(size_t)i * stride] = (i / N + (N - NL) == i % N) ? 1.0 : 0.0;
    #pragma unroll 1
    for (int s = 0; s < sweeps; ++s) gfw_pe_sweep<N, NL>(A, V, VL, stride);
}
#define GFW_PE_LDS_ROWS 4           // rows of a 9 x 9 eigenvector matrix kept behind VL: 36 doubles a lane, 73 728 B a workgroup of 256 lanes
// E: the eigenvector of the smallest eigenvalue of the moment matrix M (45, destroyed), the first of equal ones; VL: room for GFW_PE_LDS_ROWS x 9 doubles at `stride`
GFW_HD void gfw_pe_null_vector(double *M, double *E, double *VL, int stride) {
    double V[(9 - GFW_PE_LDS_ROWS) * 9];
    gfw_pe_jacobi<9, GFW_PE_LDS_ROWS>(M, V, VL, stride, GFW_PE_SWEEPS9);
    double low = M[0];
    int at = 0;
    #pragma unroll
    for (int k = 0; k < 9 - GFW_PE_LDS_ROWS; ++k) E[k] = V[k * 9];
    #pragma unroll
    for (int i = 1; i < 9; ++i) {
        const bool c = M[GFW_PE_TRI(9, i, i)] < low;
        low = c ? M[GFW_PE_TRI(9, i, i)] : low;
        at = c ? i : at;
        #pragma unroll
        for (int k = 0; k < 9 - GFW_PE_LDS_ROWS; ++k) E[k] = c ? V[k * 9 + i] : E[k];
    }
    #pragma unroll
    for (int k = 0; k < GFW_PE_LDS_ROWS; ++k) E[9 - GFW_PE_LDS_ROWS + k] = VL[(size_t)(k * 9 + at) * stride];      // (memory may be indexed by a run-time value)
}
// the squared Sampson distance of a point's normalised (x1, y1, 1), (x2, y2, 1) under E
GFW_HD double gfw_pe_sampson(const double *E, const float4 u) {
    const double x1 = (double)u.x, y1 = (double)u.y, x2 = (double)u.z, y2 = (double)u.w;
    const double l0 = ((E[0] * x1) + (E[1] * y1)) + E[2], l1 = ((E[3] * x1) + (E[4] * y1)) + E[5], l2 = ((E[6] * x1) + (E[7] * y1)) + E[8];      // E x1
    const double m0 = ((E[0] * x2) + (E[3] * y2)) + E[6], m1 = ((E[1] * x2) + (E[4] * y2)) + E[7];                                               // E^T x2
    const double r = ((x2 * l0) + (y2 * l1)) + l2;
    return (r * r) / ((((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1));
}
GFW_HD void gfw_pe_cross(const double *a, const double *b, double *o) {
    o[0] = (a[1] * b[2]) - (a[2] * b[1]); o[1] = (a[2] * b[0]) - (a[0] * b[2]); o[2] = (a[0] * b[1]) - (a[1] * b[0]);
}
// The two rotations of E and the translation direction: the SVD of E through the Jacobi eigenvectors of E^T E, U = [u1 u2 u1 x u2], V = [v1 v2 v1 x v2] (both of
// determinant +1), Ra = U W V^T, Rb = U W^T V^T, t = u3
GFW_HD void gfw_pe_rotations(const double *E, double *Ra, double *Rb, double *t) {
    double G[6], V[9];
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
        #pragma unroll
        for (int k = j; k < 3; ++k) G[GFW_PE_TRI(3, j, k)] = ((E[j] * E[k]) + (E[3 + j] * E[3 + k])) + (E[6 + j] * E[6 + k]);
    }
    gfw_pe_jacobi<3, 0>(G, V, nullptr, 0, GFW_PE_SWEEPS3);
    double lam[3] = {G[0], G[3], G[5]};
    double col[3][3];
    #pragma unroll
    for (int i = 0; i < 3; ++i) {
        #pragma unroll
        for (int k = 0; k < 3; ++k) col[i][k] = V[k * 3 + i];
    }
    const int order[3][2] = {{0, 1}, {1, 2}, {0, 1}};                                // descending, a swap only where strictly larger
    #pragma unroll
    for (int n = 0; n < 3; ++n) {
        const int i = order[n][0], j = order[n][1];
        const bool c = lam[j] > lam[i];
        const double li = lam[i], lj = lam[j];
        lam[i] = c ? lj : li; lam[j] = c ? li : lj;
        #pragma unroll
        for (int k = 0; k < 3; ++k) { const double a = col[i][k], b = col[j][k]; col[i][k] = c ? b : a; col[j][k] = c ? a : b; }
    }
    double v3[3], u[2][3], u3[3];
    gfw_pe_cross(col[0], col[1], v3);
    #pragma unroll
    for (int n = 0; n < 2; ++n) {
        double w[3];
        #pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = ((E[3 * i] * col[n][0]) + (E[3 * i + 1] * col[n][1])) + (E[3 * i + 2] * col[n][2]);
        const double len = __builtin_sqrt(((w[0] * w[0]) + (w[1] * w[1])) + (w[2] * w[2]));
        u[n][0] = w[0] / len; u[n][1] = w[1] / len; u[n][2] = w[2] / len;
    }
    gfw_pe_cross(u[0], u[1], u3);
    #pragma unroll
    for (int i = 0; i < 3; ++i) {
        #pragma unroll
        for (int j = 0; j < 3; ++j) {
            Ra[i * 3 + j] = ((u[1][i] * col[0][j]) - (u[0][i] * col[1][j])) + (u3[i] * v3[j]);
            Rb[i * 3 + j] = ((u[0][i] * col[1][j]) - (u[1][i] * col[0][j])) + (u3[i] * v3[j]);
        }
        t[i] = u3[i];
    }
}
// The numerators of a point's two depths under (R, t): z1 = n1 / det, z2 = n2 / det of the least-squares z1 R x1 - z2 x2 = -t, det = aa bb - ab^2 >= 0; under
// (R, -t) both change sign
GFW_HD void gfw_pe_depths(const double *R, const double *t, const float4 u, double &n1, double &n2) {
    const double x1 = (double)u.x, y1 = (double)u.y, x2 = (double)u.z, y2 = (double)u.w;
    const double a0 = ((R[0] * x1) + (R[1] * y1)) + R[2], a1 = ((R[3] * x1) + (R[4] * y1)) + R[5], a2 = ((R[6] * x1) + (R[7] * y1)) + R[8];
    const double aa = ((a0 * a0) + (a1 * a1)) + (a2 * a2), ab = ((a0 * x2) + (a1 * y2)) + a2, bb = ((x2 * x2) + (y2 * y2)) + 1.0;
    const double at = ((a0 * t[0]) + (a1 * t[1])) + (a2 * t[2]), bt = ((x2 * t[0]) + (y2 * t[1])) + t[2];
    n1 = (ab * bt) - (at * bb); n2 = (aa * bt) - (ab * at);
}
// R (row-major f64) -> (w, i, j, k) f32: the four-branch form, sqrt only
GFW_HD void gfw_pe_quat(const double *R, float *q) {
    const double tr = (R[0] + R[4]) + R[8];
    double w, i, j, k;
    if (tr > 0.0) {
        const double s = __builtin_sqrt(tr + 1.0) * 2.0;
        w = 0.25 * s; i = (R[7] - R[5]) / s; j = (R[2] - R[6]) / s; k = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = __builtin_sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
        w = (R[7] - R[5]) / s; i = 0.25 * s; j = (R[1] + R[3]) / s; k = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = __builtin_sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
        w = (R[2] - R[6]) / s; i = (R[1] + R[3]) / s; j = 0.25 * s; k = (R[5] + R[7]) / s;
    } else {
        const double s = __builtin_sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
        w = (R[3] - R[1]) / s; i = (R[2] + R[6]) / s; j = (R[5] + R[7]) / s; k = 0.25 * s;
    }
    q[0] = (float)w; q[1] = (float)i; q[2] = (float)j; q[3] = (float)k;
}

// the prepare stage of `total` points; the fit stage of n_pairs x num_iters lanes; the count stage, a wave per (pair, round); one workgroup per pair.
// Zero-sized launches are skipped.
hipError_t gfw_launch_pose_ess_prepare(const gfw_kernel_params &P, const GfwCommon &C, const GfwPoseEssArgs &A, hipStream_t s);
hipError_t gfw_launch_pose_ess_fit(const GfwPoseEssArgs &A, hipStream_t s);
hipError_t gfw_launch_pose_ess_count(const GfwPoseEssArgs &A, hipStream_t s);
hipError_t gfw_launch_pose_ess_pick(const GfwPoseEssArgs &A, hipStream_t s);
