// gfw_pose.hip — Almeida pose estimation of a clip's frame pairs (src/core/synchronization/estimate_pose/almeida.rs:23-238): one camera rotation per pair of frames
// from the pair's matched optical-flow points.
//
// The reference runs per pair 200 RANSAC rounds on the host; a round fits 30 steps on 3 points with four `undistort_points` calls per point and step, then maps up to
// 1000 sampled points once more — and every one of those calls inverts the lens.  `Camera::delta` (:58-68) always calls undistort_points at the same position with
// lens_correction_amount 1.0, fov 1.0, no shifts and no mesh, so the lens inverse of a point (gfw_point_ray) and its three derivative vectors (:69-77: the rotations
// are constants) are needed ONCE per point: the prepare stage, the only one that reads the lens.  Every later `delta` is gfw_point_project — one f32 gemv and two
// divides — through f32(K * f64(R)).  A fit is a lane (pair, round): 30 dependent steps on 3 points in registers.  A count is a wave (pair, round) whose lanes go over
// the round's sample list; inliers are counted by ballot.  A workgroup per pair then finds the first maximal round, packs its inliers in list order and refits on
// them: lanes write a point's products, one lane per sum folds them sequentially — the reference's `sum::<f32>()` in the order of the point list.
// The random draws (the three points of a round, its sample list) are inputs: the reference's come from an unseeded generator.
// Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; control flow around the barriers is workgroup-uniform, around the ballots wave-uniform.
#include <hip/hip_runtime.h>
#include "gfw_pose.h"
#include "gfw_points.h"

// Camera::delta (:58-68) from the prepare stage's ray: `(pt / (vw, vh)) - pos`, pt = (-1e6, -1e6) where the lens inverse is None (cpu_undistort.rs:855)
__device__ __forceinline__ float2 gfw_pose_delta(const float4 ray, const float *M, float px, float py, float vw, float vh) {
    float2 pt = float2{-1000000.0f, -1000000.0f};
    if (ray.z != 0.0f) pt = gfw_point_project(ray.x, ray.y, M);
    return float2{(pt.x / vw) - px, (pt.y / vh) - py};
}
__device__ __forceinline__ float gfw_pose_dot(const float2 a, const float2 b) { return (a.x * b.x) + (a.y * b.y); }
// f32(K * f64(matrix(q)))
__device__ __forceinline__ void gfw_pose_q_to_m(const GfwPoseArgs &A, const GfwQ4 q, float *M) {
    float R[9];
    gfw_pose_qmatrix(q, R);
    gfw_pose_kr(A.K, R, M);
}
// The inlier test of one point under a round's fit (:213-224)
__device__ __forceinline__ bool gfw_pose_inlier(const GfwPoseArgs &A, const float *M, int at) {
    const float4 pm = A.pm[at];
    const float2 d = gfw_pose_delta(A.rays[at], M, pm.x, pm.y, A.vw, A.vh);
    const float sx = pm.x + d.x, sy = pm.y + d.y, vx = pm.z - d.x, vy = pm.w - d.y;
    const float ax = gfw_atanf((sx - A.cx) / A.fx), ay = gfw_atanf((sy - A.cy) / A.fy);       // point_angle (:46-57): the normalised sample against K, as written
    const float ex = vx * gfw_cosf(ax), ey = vy * gfw_cosf(ay);
    return ((ex * ex) + (ey * ey)) <= (A.target * A.target);
}

// Prepare stage: one lane per point (workgroups of 64 x 4 lanes)
template <int MODEL>
__global__ __launch_bounds__(GFW_POSE_LANES) void gfw_pose_prepare_kernel(const gfw_kernel_params P, const GfwCommon C, const GfwPoseArgs A) {
    const int i = (int)(blockIdx.x * (unsigned)GFW_POSE_LANES + threadIdx.y * 64u + threadIdx.x);
    if (i >= A.total) return;
    const float ax = A.points[(size_t)i * 2], ay = A.points[(size_t)i * 2 + 1];
    const float bx = A.points[((size_t)A.total + i) * 2], by = A.points[((size_t)A.total + i) * 2 + 1];
    const float px = ax / A.fw, py = ay / A.fh;                                      // :28-30
    const float mx = (bx - ax) / A.fw, my = (by - ay) / A.fh;
    float ptx = 0.0f, pty = 0.0f;
    const bool ok = gfw_point_ray<MODEL>(P, C, px * A.vw, py * A.vh, ptx, pty);       // :65
    const float4 ray = float4{ptx, pty, ok ? 1.0f : 0.0f, 0.0f};
    A.pm[i] = float4{px, py, mx, my};
    A.rays[i] = ray;
    #pragma unroll
    for (int k = 0; k < 3; ++k) A.derivs[(size_t)i * 3 + k] = gfw_pose_delta(ray, A.eps_m + 9 * k, px, py, A.vw, A.vh);
}

// Fit stage: round blockIdx.x * 256 + lane of pair blockIdx.y — solve_ypr_given (:124-192) on the round's three points
__global__ __launch_bounds__(GFW_POSE_LANES) void gfw_pose_fit_kernel(const GfwPoseArgs A) {
    const int pair = (int)blockIdx.y;
    const int it = (int)(blockIdx.x * (unsigned)GFW_POSE_LANES + threadIdx.y * 64u + threadIdx.x);
    if (it >= A.num_iters) return;
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    const size_t slot = (size_t)pair * A.num_iters + it;
    GfwQ4 q = GfwQ4{1.0f, 0.0f, 0.0f, 0.0f};
    if (n >= 3) {
        float4 pm[3], ray[3];
        float2 v[3][3];
        #pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int at = first + A.triples[slot * 3 + p];
            pm[p] = A.pm[at]; ray[p] = A.rays[at];
            #pragma unroll
            for (int k = 0; k < 3; ++k) v[p][k] = A.derivs[(size_t)at * 3 + k];
        }
        float a[9];
        #pragma unroll
        for (int r = 0; r < 3; ++r) {
            #pragma unroll
            for (int c = 0; c < 3; ++c) {
                float s = 0.0f;
                #pragma unroll
                for (int p = 0; p < 3; ++p) s = s + gfw_pose_dot(v[p][c], v[p][r]);
                a[r * 3 + c] = s;
            }
        }
        const GfwLu3 L = gfw_pose_lu(a);
        #pragma unroll 1
        for (int step = 0; step < GFW_POSE_STEPS; ++step) {
            float M[9];
            gfw_pose_q_to_m(A, q, M);
            float b[3] = {0.0f, 0.0f, 0.0f};
            #pragma unroll
            for (int p = 0; p < 3; ++p) {
                const float2 d = gfw_pose_delta(ray[p], M, pm[p].x, pm[p].y, A.vw, A.vh);
                const float2 v0 = float2{pm[p].z - d.x, pm[p].w - d.y};
                #pragma unroll
                for (int r = 0; r < 3; ++r) b[r] = b[r] + gfw_pose_dot(v[p][r], v0);
            }
            q = gfw_pose_update(q, L, b[0], b[1], b[2], step == GFW_POSE_STEPS - 1 ? 1.0f : 0.5f);
        }
    }
    float *o = A.fits + slot * 4;
    o[0] = q.w; o[1] = q.i; o[2] = q.j; o[3] = q.k;
}

// The sample list of a round: entry s of the pair's `m` is samples[sample_first[pair] + it * m + s], or s itself without lists
__device__ __forceinline__ int gfw_pose_sample(const GfwPoseArgs &A, int pair, int it, int m, int s) {
    return A.samples ? A.samples[(size_t)A.sample_first[pair] + (size_t)it * m + s] : s;
}

// Count stage: round blockIdx.x * 4 + wave of pair blockIdx.y
__global__ __launch_bounds__(GFW_POSE_LANES) void gfw_pose_count_kernel(const GfwPoseArgs A) {
    const int pair = (int)blockIdx.y;
    const int it = (int)(blockIdx.x * 4u + threadIdx.y), lane = (int)threadIdx.x;
    if (it >= A.num_iters) return;                                                   // wave-uniform
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    const size_t slot = (size_t)pair * A.num_iters + it;
    int count = 0;
    if (n >= 3) {                                                                    // wave-uniform
        const float *f = A.fits + slot * 4;
        float M[9];
        gfw_pose_q_to_m(A, GfwQ4{f[0], f[1], f[2], f[3]}, M);
        const int m = n < A.num_samples ? n : A.num_samples;
        for (int base = 0; base < m; base += 64) {
            const int s = base + lane;
            const bool in = s < m && gfw_pose_inlier(A, M, first + gfw_pose_sample(A, pair, it, m, s));
            count += (int)__popcll(__ballot(in));
        }
    }
    if (lane == 0) A.counts[slot] = count;
}

// The f32 sums of a point list by a workgroup: lane t writes the `K` products of point base + t, lane k < K folds column k in list order
template <int K, typename Products>
__device__ __forceinline__ void gfw_pose_fold(const Products &products, int t, int n, float (*s_prod)[GFW_POSE_LANES], float *s_sum) {
    float acc = 0.0f;
    for (int base = 0; base < n; base += GFW_POSE_LANES) {
        if (base + t < n) {
            float pr[K];
            products(base + t, pr);
            #pragma unroll
            for (int k = 0; k < K; ++k) s_prod[k][t] = pr[k];
        }
        __syncthreads();
        if (t < K) {
            const int cnt = n - base < GFW_POSE_LANES ? n - base : GFW_POSE_LANES;
            for (int j = 0; j < cnt; ++j) acc = acc + s_prod[t][j];
        }
        __syncthreads();
    }
    if (t < K) s_sum[t] = acc;
    __syncthreads();
}

// Pick-and-refit stage: workgroup blockIdx.x is a pair (:228-237)
__global__ __launch_bounds__(GFW_POSE_LANES) void gfw_pose_pick_kernel(const GfwPoseArgs A) {
    __shared__ int s_cnt[GFW_POSE_LANES], s_rnd[GFW_POSE_LANES];
    __shared__ uint16_t s_idx[GFW_POSE_PAIR_MAX];
    __shared__ float s_prod[6][GFW_POSE_LANES];
    __shared__ float s_sum[6];
    __shared__ int s_pick[2];
    const int pair = (int)blockIdx.x;
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    // the first maximal round: `if inliers.len() > best_inliers.len()` in round order
    int cnt = -1, rnd = -1;
    for (int c = t; c < A.num_iters; c += GFW_POSE_LANES) {
        const int v = A.counts[(size_t)pair * A.num_iters + c];
        if (v > cnt) { cnt = v; rnd = c; }
    }
    s_cnt[t] = cnt; s_rnd[t] = rnd;
    __syncthreads();
    if (t == 0) {
        int bc = 0, br = -1;
        for (int j = 0; j < GFW_POSE_LANES; ++j)
            if (s_rnd[j] >= 0 && (br < 0 || s_cnt[j] > bc || (s_cnt[j] == bc && s_rnd[j] < br))) { bc = s_cnt[j]; br = s_rnd[j]; }
        s_pick[0] = bc; s_pick[1] = br;
    }
    __syncthreads();
    const int n_in = s_pick[0], round = s_pick[1];
    GfwQ4 q = GfwQ4{1.0f, 0.0f, 0.0f, 0.0f};
    if (n_in >= 3) {                                                                 // workgroup-uniform
        if (t < 64) {                                                                // the first wave packs the round's inliers in list order
            const float *f = A.fits + ((size_t)pair * A.num_iters + round) * 4;
            float M[9];
            gfw_pose_q_to_m(A, GfwQ4{f[0], f[1], f[2], f[3]}, M);
            const int m = n < A.num_samples ? n : A.num_samples;
            int packed = 0;
            for (int base = 0; base < m; base += 64) {
                const int s = base + t;
                const int idx = s < m ? gfw_pose_sample(A, pair, round, m, s) : 0;
                const bool in = s < m && gfw_pose_inlier(A, M, first + idx);
                const unsigned long long mask = __ballot(in);
                if (in) s_idx[packed + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u))] = (uint16_t)idx;
                packed += (int)__popcll(mask);
            }
        }
        __syncthreads();
        // solve_ypr_given over the inliers: the matrix does not depend on the step
        const auto mat = [&](int p, float *pr) {
            const float2 *v = A.derivs + (size_t)(first + s_idx[p]) * 3;
            const float2 v1 = v[0], v2 = v[1], v3 = v[2];
            pr[0] = gfw_pose_dot(v1, v1); pr[1] = gfw_pose_dot(v2, v1); pr[2] = gfw_pose_dot(v3, v1);
            pr[3] = gfw_pose_dot(v2, v2); pr[4] = gfw_pose_dot(v3, v2); pr[5] = gfw_pose_dot(v3, v3);
        };
        gfw_pose_fold<6>(mat, t, n_in, s_prod, s_sum);
        const float a[9] = {s_sum[0], s_sum[1], s_sum[2], s_sum[1], s_sum[3], s_sum[4], s_sum[2], s_sum[4], s_sum[5]};       // dot(a, b) = dot(b, a) to the bit
        const GfwLu3 L = gfw_pose_lu(a);
        __syncthreads();
        #pragma unroll 1
        for (int step = 0; step < GFW_POSE_STEPS; ++step) {
            float M[9];
            gfw_pose_q_to_m(A, q, M);
            const auto rhs = [&](int p, float *pr) {
                const int at = first + s_idx[p];
                const float4 pm = A.pm[at];
                const float2 d = gfw_pose_delta(A.rays[at], M, pm.x, pm.y, A.vw, A.vh);
                const float2 v0 = float2{pm.z - d.x, pm.w - d.y};
                const float2 *v = A.derivs + (size_t)at * 3;
                pr[0] = gfw_pose_dot(v[0], v0); pr[1] = gfw_pose_dot(v[1], v0); pr[2] = gfw_pose_dot(v[2], v0);
            };
            gfw_pose_fold<3>(rhs, t, n_in, s_prod, s_sum);
            q = gfw_pose_update(q, L, s_sum[0], s_sum[1], s_sum[2], step == GFW_POSE_STEPS - 1 ? 1.0f : 0.5f);
            __syncthreads();
        }
    }
    if (t == 0) {
        float R[9];
        gfw_pose_qmatrix(q, R);
        float *o = A.quats + (size_t)pair * 4;
        o[0] = q.w; o[1] = q.i; o[2] = q.j; o[3] = q.k;
        for (int k = 0; k < 9; ++k) A.rotations[(size_t)pair * 9 + k] = (double)R[k];
        A.best[pair * 2] = n_in; A.best[pair * 2 + 1] = round;
    }
}

hipError_t gfw_launch_pose_prepare(const gfw_kernel_params &P, const GfwCommon &C, const GfwPoseArgs &A, hipStream_t s) {
    if (A.total <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((size_t)A.total + GFW_POSE_LANES - 1) / GFW_POSE_LANES));
    if (C.model == GFW_MODEL_OPENCV_FISHEYE) hipLaunchKernelGGL(gfw_pose_prepare_kernel<GFW_MODEL_OPENCV_FISHEYE>, grid, dim3(64, 4), 0, s, P, C, A);
    else hipLaunchKernelGGL(gfw_pose_prepare_kernel<-1>, grid, dim3(64, 4), 0, s, P, C, A);
    return hipGetLastError();
}
hipError_t gfw_launch_pose_fit(const GfwPoseArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0 || A.num_iters <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_pose_fit_kernel, dim3((unsigned)((A.num_iters + GFW_POSE_LANES - 1) / GFW_POSE_LANES), (unsigned)A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_pose_count(const GfwPoseArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0 || A.num_iters <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_pose_count_kernel, dim3((unsigned)((A.num_iters + 3) / 4), (unsigned)A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_pose_pick(const GfwPoseArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_pose_pick_kernel, dim3((unsigned)A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
