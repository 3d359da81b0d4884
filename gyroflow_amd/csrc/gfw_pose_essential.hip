// gfw_pose_essential.hip — essential-matrix pose estimation of a clip's frame pairs: one camera rotation per pair from the pair's matched optical-flow points, where
// the camera also moved (what the reference's pose methods 0 and 2 are for; gfw_pose_essential.h says what of them is not reproduced).
//
// Four stages.  Prepare: a lane per point inverts the lens for both of its frames (gfw_point_ray, called as gfw_pose.hip's prepare stage calls it: identity rotation,
// no P, correction amount 1.0, fov 1.0) — the only stage that reads the lens.  Fit: a lane is a (pair, round): the 9 x 9 moment matrix of the round's 8 bearings
// and its eigenvector of the smallest eigenvalue by a cyclic Jacobi iteration, the triangle and five rows of the eigenvectors in the lane's registers, four rows in its
// column of LDS (two waves a SIMD).  Count: a wave per (pair, round)
// goes over the pair's points, inliers (squared Sampson distance) counted by ballot.  Pick: a workgroup per pair finds the first maximal round, packs its inliers in
// point order, folds their moment matrix column by column in list order, solves once more, decomposes E and counts the inliers in front of both cameras.
// All arithmetic behind the prepare stage is f64 (+ - * / sqrt).  Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; control flow around the
// barriers is workgroup-uniform, around the ballots wave-uniform.
#include <hip/hip_runtime.h>
#include "gfw_pose_essential.h"
#include "gfw_points.h"

// the lens inverse of a flow-image point; (-1e6, -1e6) where it is None
template <int MODEL>
__device__ __forceinline__ float2 gfw_pe_undistort(const gfw_kernel_params &P, const GfwCommon &C, const GfwPoseEssArgs &A, float x, float y) {
    const float px = x / A.fw, py = y / A.fh;
    float ptx = 0.0f, pty = 0.0f;
    const bool ok = gfw_point_ray<MODEL>(P, C, px * A.vw, py * A.vh, ptx, pty);
    return ok ? float2{ptx, pty} : float2{GFW_PE_NONE, GFW_PE_NONE};
}

// Prepare stage: one lane per point (workgroups of 64 x 4 lanes)
template <int MODEL>
__global__ __launch_bounds__(GFW_PE_LANES) void gfw_pe_prepare_kernel(const gfw_kernel_params P, const GfwCommon C, const GfwPoseEssArgs A) {
    const int i = (int)(blockIdx.x * (unsigned)GFW_PE_LANES + threadIdx.y * 64u + threadIdx.x);
    if (i >= A.total) return;
    const float2 a = gfw_pe_undistort<MODEL>(P, C, A, A.points[(size_t)i * 2], A.points[(size_t)i * 2 + 1]);
    const float2 b = gfw_pe_undistort<MODEL>(P, C, A, A.points[((size_t)A.total + i) * 2], A.points[((size_t)A.total + i) * 2 + 1]);
    A.und[i] = float4{a.x, a.y, b.x, b.y};
}

// Fit stage: round blockIdx.x * 256 + lane of pair blockIdx.y
__global__ __launch_bounds__(GFW_PE_LANES) void gfw_pe_fit_kernel(const GfwPoseEssArgs A) {
    __shared__ double s_v[GFW_PE_LDS_ROWS * 9][GFW_PE_LANES];                        // a lane's column: the last rows of its eigenvector matrix (no lane reads another's)
    const int pair = (int)blockIdx.y;
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int it = (int)(blockIdx.x * (unsigned)GFW_PE_LANES) + t;
    if (it >= A.num_iters) return;
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    const size_t slot = (size_t)pair * A.num_iters + it;
    double E[9];
    #pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0.0;
    if (n >= GFW_PE_MIN_POINTS) {
        double M[45];
        #pragma unroll
        for (int k = 0; k < 45; ++k) M[k] = 0.0;
        #pragma unroll 1
        for (int p = 0; p < GFW_PE_MIN_POINTS; ++p) {
            double a[9];
            gfw_pe_kron(A.und[first + A.octets[slot * GFW_PE_MIN_POINTS + p]], a);
            #pragma unroll
            for (int i = 0; i < 9; ++i) {
                #pragma unroll
                for (int j = i; j < 9; ++j) M[GFW_PE_TRI(9, i, j)] = M[GFW_PE_TRI(9, i, j)] + (a[i] * a[j]);
            }
        }
        gfw_pe_null_vector(M, E, &s_v[0][t], GFW_PE_LANES);
    }
    double *o = A.fits + slot * 9;
    #pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = E[k];
}

// Count stage: round blockIdx.x * 4 + wave of pair blockIdx.y
__global__ __launch_bounds__(GFW_PE_LANES) void gfw_pe_count_kernel(const GfwPoseEssArgs A) {
    const int pair = (int)blockIdx.y;
    const int it = (int)(blockIdx.x * 4u + threadIdx.y), lane = (int)threadIdx.x;
    if (it >= A.num_iters) return;                                                   // wave-uniform
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    const size_t slot = (size_t)pair * A.num_iters + it;
    int count = 0;
    if (n >= GFW_PE_MIN_POINTS) {                                                    // wave-uniform
        double E[9];
        #pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = A.fits[slot * 9 + k];
        for (int base = 0; base < n; base += 64) {
            const int s = base + lane;
            const bool in = s < n && gfw_pe_sampson(E, A.und[first + s]) <= A.threshold;
            count += (int)__popcll(__ballot(in));
        }
    }
    if (lane == 0) A.counts[slot] = count;
}

// Pick-and-refit stage: workgroup blockIdx.x is a pair
__global__ __launch_bounds__(GFW_PE_LANES) void gfw_pe_pick_kernel(const GfwPoseEssArgs A) {
    __shared__ int s_cnt[GFW_PE_LANES], s_rnd[GFW_PE_LANES];
    __shared__ uint16_t s_idx[GFW_PE_PAIR_MAX];
    __shared__ double s_prod[45][64];
    __shared__ double s_sum[45];
    __shared__ int s_pick[2];
    __shared__ int s_front[4][4];
    __shared__ double s_v[GFW_PE_LDS_ROWS * 9][GFW_PE_LANES];                        // a lane's column: the last rows of its eigenvector matrix
    const int pair = (int)blockIdx.x;
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    // the first maximal round
    int cnt = -1, rnd = -1;
    for (int c = t; c < A.num_iters; c += GFW_PE_LANES) {
        const int v = A.counts[(size_t)pair * A.num_iters + c];
        if (v > cnt) { cnt = v; rnd = c; }
    }
    s_cnt[t] = cnt; s_rnd[t] = rnd;
    __syncthreads();
    if (t == 0) {
        int bc = 0, br = -1;
        for (int j = 0; j < GFW_PE_LANES; ++j)
            if (s_rnd[j] >= 0 && (br < 0 || s_cnt[j] > bc || (s_cnt[j] == bc && s_rnd[j] < br))) { bc = s_cnt[j]; br = s_rnd[j]; }
        s_pick[0] = bc; s_pick[1] = br;
    }
    __syncthreads();
    const int n_in = s_pick[0], round = s_pick[1];
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double E[9];
    #pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0.0;
    int front = 0, found = 0;
    if (n_in >= GFW_PE_MIN_POINTS) {                                                 // workgroup-uniform
        if (t < 64) {                                                                // the first wave packs the round's inliers in point order
            double F[9];
            #pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = A.fits[((size_t)pair * A.num_iters + round) * 9 + k];
            int packed = 0;
            for (int base = 0; base < n; base += 64) {
                const int s = base + t;
                const bool in = s < n && gfw_pe_sampson(F, A.und[first + s]) <= A.threshold;
                const unsigned long long mask = __ballot(in);
                if (in) s_idx[packed + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u))] = (uint16_t)s;
                packed += (int)__popcll(mask);
            }
        }
        __syncthreads();
        // the moment matrix over the inliers: lane t < 64 writes the 45 products of point base + t, lane k < 45 folds column k in list order
        double acc = 0.0;
        for (int base = 0; base < n_in; base += 64) {
            if (t < 64 && base + t < n_in) {
                double a[9];
                gfw_pe_kron(A.und[first + s_idx[base + t]], a);
                #pragma unroll
                for (int i = 0; i < 9; ++i) {
                    #pragma unroll
                    for (int j = i; j < 9; ++j) s_prod[GFW_PE_TRI(9, i, j)][t] = a[i] * a[j];
                }
            }
            __syncthreads();
            if (t < 45) {
                const int c = n_in - base < 64 ? n_in - base : 64;
                for (int j = 0; j < c; ++j) acc = acc + s_prod[t][j];
            }
            __syncthreads();
        }
        if (t < 45) s_sum[t] = acc;
        __syncthreads();
        // every lane solves and decomposes alike: the rotations are needed by all of them
        double M[45];
        #pragma unroll
        for (int k = 0; k < 45; ++k) M[k] = s_sum[k];
        gfw_pe_null_vector(M, E, &s_v[0][t], GFW_PE_LANES);
        double Ra[9], Rb[9], tv[3];
        gfw_pe_rotations(E, Ra, Rb, tv);
        int f[4] = {0, 0, 0, 0};                                                     // Ra with +t, -t; Rb with +t, -t
        for (int base = 0; base < n_in; base += GFW_PE_LANES) {
            const int s = base + t;
            double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
            if (s < n_in) {
                const float4 u = A.und[first + s_idx[s]];
                gfw_pe_depths(Ra, tv, u, a1, a2);
                gfw_pe_depths(Rb, tv, u, b1, b2);
            }
            f[0] += (int)__popcll(__ballot(a1 > 0.0 && a2 > 0.0)); f[1] += (int)__popcll(__ballot(a1 < 0.0 && a2 < 0.0));
            f[2] += (int)__popcll(__ballot(b1 > 0.0 && b2 > 0.0)); f[3] += (int)__popcll(__ballot(b1 < 0.0 && b2 < 0.0));
        }
        if (threadIdx.x == 0) { s_front[threadIdx.y][0] = f[0]; s_front[threadIdx.y][1] = f[1]; s_front[threadIdx.y][2] = f[2]; s_front[threadIdx.y][3] = f[3]; }
        __syncthreads();
        #pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = ((s_front[0][k] + s_front[1][k]) + s_front[2][k]) + s_front[3][k];
        const int sa = f[0] > f[1] ? f[0] : f[1], sb = f[2] > f[3] ? f[2] : f[3];
        const double tra = (Ra[0] + Ra[4]) + Ra[8], trb = (Rb[0] + Rb[4]) + Rb[8];
        const bool use_b = sb > sa || (sb == sa && trb > tra);                       // the higher count; equal counts: the larger trace (the smaller angle)
        front = use_b ? sb : sa;
        found = front >= A.min_front ? 1 : 0;
        if (found) {
            #pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = use_b ? Rb[k] : Ra[k];
        }
    }
    if (t == 0) {
        float q[4];
        gfw_pe_quat(R, q);
        float *o = A.quats + (size_t)pair * 4;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
        for (int k = 0; k < 9; ++k) { A.rotations[(size_t)pair * 9 + k] = R[k]; A.essential[(size_t)pair * 9 + k] = E[k]; }
        int32_t *b = A.best + (size_t)pair * 4;
        b[0] = n_in; b[1] = round; b[2] = front; b[3] = found;
    }
}

hipError_t gfw_launch_pose_ess_prepare(const gfw_kernel_params &P, const GfwCommon &C, const GfwPoseEssArgs &A, hipStream_t s) {
    if (A.total <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((size_t)A.total + GFW_PE_LANES - 1) / GFW_PE_LANES));
    if (C.model == GFW_MODEL_OPENCV_FISHEYE) hipLaunchKernelGGL(gfw_pe_prepare_kernel<GFW_MODEL_OPENCV_FISHEYE>, grid, dim3(64, 4), 0, s, P, C, A);
    else hipLaunchKernelGGL(gfw_pe_prepare_kernel<-1>, grid, dim3(64, 4), 0, s, P, C, A);
    return hipGetLastError();
}
hipError_t gfw_launch_pose_ess_fit(const GfwPoseEssArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0 || A.num_iters <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_pe_fit_kernel, dim3((unsigned)((A.num_iters + GFW_PE_LANES - 1) / GFW_PE_LANES), (unsigned)A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_pose_ess_count(const GfwPoseEssArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0 || A.num_iters <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_pe_count_kernel, dim3((unsigned)((A.num_iters + 3) / 4), (unsigned)A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_pose_ess_pick(const GfwPoseEssArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_pe_pick_kernel, dim3((unsigned)A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
