// gfw_sync.hip — the "visual features" offset search (src/core/synchronization/find_offset/visual_features.rs:10-147; with for_rs the rolling-shutter estimator).
//
// The reference evaluates calculate_distance (:49-83) for search_size coarse and 200 fine candidates of a range under rayon on the host: per candidate and matched frame
// pair both point sets go through undistort_points_with_rolling_shutter at `timestamp - offs`, and the 90 % shortest squared distances are summed.  Candidates and pairs
// are independent, so here a (candidate, pair) is a workgroup — one wave whose lanes stride over the pair's points.  What does not depend on the candidate (the lens
// inverse of every point: gfw_point_ray) runs once per call in a stage of its own; per candidate a point costs its rotation (the f64 slerp of gfw_zoom_rotation under
// rolling shutter), an f32 gemv and a divide.
//
// The fold needs no sort: every distance is `dist as u64` of an f32 below 2^32 and the totals stay far below 2^53, so sums are exact and order-free, and the sum of the
// k smallest of a set is  sum(d < T) + (k - count(d < T)) * T  for its k-th smallest value T — found by bisection over counts (__ballot + popcount); ties at T cost
// nothing.  A pair's u64 goes to partial[candidate][pair]; the reduce stage adds a candidate's pairs, converts once (= the reference's sequential f64 adds of
// integers) and picks the minimum the way `reduce_with(find_min)` does: `if a.1 < b.1 { a } else { b }` under an order-preserving reduce — the LAST minimal candidate.
// All stores are ordinary vector stores; control flow around the barriers is workgroup-uniform.
#include <hip/hip_runtime.h>
#include "gfw_sync.h"
#include "gfw_points.h"
#include "gfw_quat.h"

// Lens stage: one lane per point of either side (workgroups of 64 x 4 lanes)
template <int MODEL>
__global__ __launch_bounds__(256) void gfw_sync_rays_kernel(const gfw_kernel_params P, const GfwCommon C, const GfwSyncArgs A) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x);
    if (i >= A.total * 2) return;
    float ptx = 0.0f, pty = 0.0f;
    const bool ok = gfw_point_ray<MODEL>(P, C, A.points[(size_t)i * 2], A.points[(size_t)i * 2 + 1], ptx, pty);
    A.rays[i] = float4{ptx, pty, ok ? 1.0f : 0.0f, 0.0f};
}

// The fold of one pair (:66-81) by the 64 lanes t of a wave: map(i) -> point pair i as mapped, (p1.x, p1.y, p2.x, p2.y).  s_dist: room for the pair's valid distances,
// packed in point order; -> the sum of the k = (n_valid as f64 * 0.9) as usize smallest (every lane's value).
template <typename Map>
__device__ __forceinline__ unsigned long long gfw_sync_fold(const Map &map, int t, int n, float w, float h, uint32_t *s_dist, unsigned long long *s_sum) {
    if (t == 0) *s_sum = 0ull;
    int n_valid = 0;
    for (int base = 0; base < n; base += GFW_SYNC_LANES) {
        const int i = base + t;
        bool valid = false;
        uint32_t d = 0u;
        if (i < n) {
            const float4 o = map(i);
            valid = o.x > 0.0f && o.x < w && o.y > 0.0f && o.y < h && o.z > 0.0f && o.z < w && o.w > 0.0f && o.w < h;            // :68-69
            const float dist = ((o.z - o.x) * (o.z - o.x)) + ((o.w - o.y) * (o.w - o.y));                                      // :70-71
            d = valid ? (uint32_t)dist : 0u;                                         // `dist as u64`: below 2^32 inside the frame
        }
        const unsigned long long mask = __ballot(valid);
        if (valid) s_dist[n_valid + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u))] = d;
        n_valid += (int)__popcll(mask);
    }
    __syncthreads();
    const int k = (int)((double)n_valid * 0.9);                                      // :78
    if (k <= 0) return 0ull;                                                         // workgroup-uniform
    // T = the k-th smallest: the least value with count(d <= T) >= k.  A distance inside the frame is below (w^2 + h^2) (1 + 2^-22).
    const float bound = (w * w + h * h) * 1.001f + 1.0f;
    uint32_t lo = 0u, hi = bound < 4294967040.0f ? (uint32_t)bound : 0xffffffffu;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        int cnt = 0;
        for (int base = 0; base < n_valid; base += GFW_SYNC_LANES) cnt += (int)__popcll(__ballot(base + t < n_valid && s_dist[base + t] <= mid));
        if (cnt >= k) hi = mid; else lo = mid + 1u;
    }
    unsigned long long below = 0ull;
    int cnt_below = 0;
    for (int base = 0; base < n_valid; base += GFW_SYNC_LANES) {
        const bool in = base + t < n_valid && s_dist[base + t] < lo;
        if (in) below += s_dist[base + t];
        cnt_below += (int)__popcll(__ballot(in));
    }
    if (below) atomicAdd(s_sum, below);
    __syncthreads();
    return *s_sum + (unsigned long long)(k - cnt_below) * lo;
}

// undistort_points_with_rolling_shutter of point pair i of a pair for one candidate, from the lens stage's rays
struct GfwSyncMap {
    const GfwSyncArgs &A;
    const float *s_rot; const double *s_side;        // LDS: per side the one rotation (no rolling shutter); the prefix smoothed(ts) * org(ts)^-1 and ts - readout / 2
    size_t cand; int first; bool rolling;
    double row_readout_time;
    __device__ __forceinline__ float4 operator()(int i) const {
        float2 o0 = float2{0.0f, 0.0f}, o1 = o0;
        #pragma unroll 1
        for (int s = 0; s < 2; ++s) {                                                // (one body for both sides: the rotation's f64 code is not duplicated)
            const size_t at = (size_t)s * A.total + first + i;
            const float4 ray = A.rays[at];
            float2 o = float2{-1000000.0f, -1000000.0f};                             // cpu_undistort.rs:855
            if (ray.z != 0.0f) {
                float rot[9];
                if (rolling) {
                    const float x = A.points[at * 2], y = A.points[at * 2 + 1];      // frame_transform.rs:393-394: the point as given
                    const double *sd = s_side + s * 5;
                    gfw_zoom_rotation(A.T, A.F, Q{sd[0], sd[1], sd[2], sd[3]}, sd[4] + row_readout_time * (double)(A.horizontal ? x : y), rot);
                } else { for (int k = 0; k < 9; ++k) rot[k] = s_rot[s * 9 + k]; }
                o = gfw_point_project(ray.x, ray.y, rot);
            }
            if (s) o1 = o; else o0 = o;
        }
        const float4 r = float4{o0.x, o0.y, o1.x, o1.y};
        if (A.mapped) { float *m = A.mapped + (cand * (size_t)A.total + first + i) * 4; m[0] = r.x; m[1] = r.y; m[2] = r.z; m[3] = r.w; }     // (f32 alignment is all it has)
        return r;
    }
};

// Cost stage: candidate blockIdx.x, pair blockIdx.y.  Nothing behind the lens stage reads the lens model (lens_correction_amount is 1.0: no blend), so there
// is one instantiation.
__global__ __launch_bounds__(GFW_SYNC_LANES) void gfw_sync_cost_kernel(const GfwSyncArgs A) {
#if defined(GFW_HOST_INTERPRETER)
    __shared__ uint32_t s_dist[GFW_SYNC_PAIR_MAX];                                    // (the host interpreter has no dynamic LDS: the largest block)
#else
    extern __shared__ uint32_t s_dist[];                                             // the call's largest pair
#endif
    __shared__ float s_rot[18];
    __shared__ double s_side[10];
    __shared__ unsigned long long s_sum;
    if (A.gate && !A.gate->found) return;                                            // workgroup-uniform
    const int t = threadIdx.x;
    const size_t cand = blockIdx.x;
    const int pair = blockIdx.y;
    const double offs = A.candidates[cand * 2], frt = A.candidates[cand * 2 + 1];
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first;
    const GfwSyncMap map{A, s_rot, s_side, cand, first, fabs(frt) > 0.0, frt / (double)A.readout_dim};
    if (t == 0) {                                                                    // once per side, not per point
        #pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            const double ts = (double)A.pair_ts[pair * 2 + s] / 1000.0 - offs;       // :60-64: `*ts as f64 / 1000.0`, then `timestamp_ms - offs`
            const double start_ts = ts - frt / 2.0;                                  // frame_transform.rs:380
            const Q pre = quat_prefix(A.T, ts);
            if (!map.rolling) gfw_zoom_rotation(A.T, A.F, pre, start_ts, s_rot + s * 9);
            double *sd = s_side + s * 5;
            sd[0] = pre.w; sd[1] = pre.x; sd[2] = pre.y; sd[3] = pre.z; sd[4] = start_ts;
        }
    }
    __syncthreads();
    const unsigned long long total = gfw_sync_fold(map, t, n, A.w, A.h, s_dist, &s_sum);
    if (t == 0) A.partial[cand * (size_t)A.n_pairs + pair] = total;
}

// Reduce stage: a candidate's cost, the stage's pick and, behind the coarse stage, the fine candidates around it (:99-103, :123-127)
__global__ __launch_bounds__(GFW_SYNC_REDUCE_LANES) void gfw_sync_reduce_kernel(const GfwSyncReduceArgs R) {
    __shared__ double s_cost[GFW_SYNC_REDUCE_LANES];
    __shared__ int s_idx[GFW_SYNC_REDUCE_LANES];
    __shared__ int s_pick;
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    if (R.stage == 1 && !R.result->found) {                                          // workgroup-uniform: a search without candidates has no second stage
        if (R.costs) for (int c = t; c < R.n; c += GFW_SYNC_REDUCE_LANES) R.costs[c] = 0.0;
        return;
    }
    double best = 0.0;
    int idx = -1;
    for (int c = t; c < R.n; c += GFW_SYNC_REDUCE_LANES) {
        unsigned long long sum = 0ull;
        for (int p = 0; p < R.n_pairs; ++p) sum += R.partial[(size_t)c * R.n_pairs + p];
        const double cost = (double)sum;
        if (R.costs) R.costs[c] = cost;
        if (idx < 0 || cost <= best) { best = cost; idx = c; }                       // of equal costs the later candidate
    }
    if (!R.result) return;
    s_cost[t] = best; s_idx[t] = idx;
    __syncthreads();
    if (t == 0) {
        int pick = -1;
        double low = 0.0;
        for (int j = 0; j < GFW_SYNC_REDUCE_LANES; ++j) {
            if (s_idx[j] < 0) continue;
            if (pick < 0 || s_cost[j] < low || (s_cost[j] == low && s_idx[j] > pick)) { low = s_cost[j]; pick = s_idx[j]; }
        }
        s_pick = pick;
        const double value = pick >= 0 ? R.candidates[(size_t)pick * 2 + R.column] : 0.0;
        if (R.stage == 0) {
            gfw_sync_result r;
            r.found = pick >= 0 ? 1 : 0; r.n_coarse = R.n;
            r.coarse_value = value; r.coarse_cost = low; r.value = 0.0; r.cost = 0.0;
            *R.result = r;
        } else if (pick >= 0) { R.result->value = value; R.result->cost = low; }
    }
    __syncthreads();
    if (R.stage == 0 && R.fine && s_pick >= 0 && t < GFW_SYNC_FINE) {
        const double lowest = R.candidates[(size_t)s_pick * 2 + R.column];
        R.fine[t * 2 + R.column] = lowest - 1.0 + ((double)t * 0.01);
        R.fine[t * 2 + (1 - R.column)] = R.candidates[(size_t)s_pick * 2 + (1 - R.column)];
    }
}

hipError_t gfw_launch_sync_rays(const gfw_kernel_params &P, const GfwCommon &C, const GfwSyncArgs &A, hipStream_t s) {
    if (A.total <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((size_t)A.total * 2 + 255) / 256));
    if (C.model == GFW_MODEL_OPENCV_FISHEYE) hipLaunchKernelGGL(gfw_sync_rays_kernel<GFW_MODEL_OPENCV_FISHEYE>, grid, dim3(64, 4), 0, s, P, C, A);
    else hipLaunchKernelGGL(gfw_sync_rays_kernel<-1>, grid, dim3(64, 4), 0, s, P, C, A);
    return hipGetLastError();
}
hipError_t gfw_launch_sync_costs(const GfwSyncArgs &A, int n, int max_pair_points, hipStream_t s) {
    if (n <= 0 || A.n_pairs <= 0) return hipSuccess;
    const dim3 grid((unsigned)n, (unsigned)A.n_pairs);
    const size_t lds = sizeof(uint32_t) * (size_t)(max_pair_points > 0 ? max_pair_points : 1);
    hipLaunchKernelGGL(gfw_sync_cost_kernel, grid, dim3(GFW_SYNC_LANES), lds, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_sync_reduce(const GfwSyncReduceArgs &R, hipStream_t s) {
    hipLaunchKernelGGL(gfw_sync_reduce_kernel, dim3(1), dim3(64, GFW_SYNC_REDUCE_LANES / 64), 0, s, R);
    return hipGetLastError();
}
