// gfw_sync_rs.hip — the rs-sync offset search of a clip's ranges (find_offset/rs_sync.rs, offset method 2; gfw_sync_rs.h says what of it is not reproduced).
//
// Three stages.  Prepare: a lane per point and side inverts the lens (gfw_point_ray, called as gfw_pose_essential.hip's prepare stage calls it), makes the f64 unit
// bearing and the point's own time, pair_ts + readout * (y / height) — the only stage that reads the lens.  Cost: a one-wave workgroup is a (candidate, pair): lanes
// stride over the pair's points, two track lookups — bisections inside the window of the pair's time span at this delay — and m = ra x rb per point, m kept in LDS
// (24 B a point); the direction hypotheses and the reweighted refits are wave reductions in the statement's order — lane-strided partial sums from 0.0, then the
// butterfly v = v + v[lane ^ off], off = 32 .. 1, which leaves the same sum in every lane (IEEE addition commutes) — and every lane solves the 3 x 3 eigenproblems
// alike.  Pick: a workgroup per range adds a candidate's pairs in pair order, takes the first minimum, writes the round's pick and the next round's 17 candidates,
// and behind the last round fits the parabola.
// All arithmetic behind the lens is f64 (+ - * / sqrt).  Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; control flow around the
// barriers is workgroup-uniform, around the shuffles wave-uniform.
#include <hip/hip_runtime.h>
#include "gfw_sync_rs.h"
#include "gfw_points.h"

#ifndef GFW_RS_DYN_LDS                                                               // (the host interpreter has no dynamic LDS: it defines a static array of the largest size)
#define GFW_RS_DYN_LDS(name) extern __shared__ double name[]
#endif

// Prepare stage: lane i is side i / total of point i % total (workgroups of 64 x 4 lanes)
template <int MODEL>
__global__ __launch_bounds__(GFW_RS_LANES) void gfw_rs_prepare_kernel(const gfw_kernel_params P, const GfwCommon C, const GfwRsArgs A) {
    const long long i = (long long)blockIdx.x * GFW_RS_LANES + threadIdx.y * 64u + threadIdx.x;
    if (i >= 2ll * A.total) return;
    const int side = i >= A.total ? 1 : 0, idx = (int)(i - (side ? A.total : 0));
    int lo = 0, hi = A.n_pairs;                                                      // the pair that owns the point: the last with pair_first <= idx
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (A.pair_first[mid] <= idx) lo = mid; else hi = mid;
    }
    const float x = A.points[(size_t)i * 2], y = A.points[(size_t)i * 2 + 1];
    const float px = x / A.fw, py = y / A.fh;
    float ptx = 0.0f, pty = 0.0f;
    const bool ok = gfw_point_ray<MODEL>(P, C, px * A.vw, py * A.vh, ptx, pty);
    double b[3];
    gfw_pe_bearing((double)(ok ? ptx : GFW_PE_NONE), (double)(ok ? pty : GFW_PE_NONE), b);
    double *o = A.prep + (size_t)i * 4;
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2];
    o[3] = ((double)A.pair_ts[(size_t)lo * 2 + side] / 1000000.0) + (A.readout_s * ((double)y / A.flow_h));      // rs_sync.rs:132-133
}

__device__ __forceinline__ int gfw_rs_cand_count(const GfwRsArgs &A, int r) { return A.mode == 0 ? A.cand_first[r + 1] - A.cand_first[r] : A.n_cand; }
__device__ __forceinline__ double gfw_rs_candidate(const GfwRsArgs &A, int r, int c) {
    if (A.mode == 0) return A.cand[(size_t)A.cand_first[r] + c];
    if (A.mode == 1) return A.initial + ((double)(c - A.half) * A.step);
    return A.cand_all[(size_t)r * A.total_cand + A.at + c];
}
__device__ __forceinline__ double gfw_rs_wave_sum(double v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}
// sum rho(k m_i . t) over the pair's points
__device__ __forceinline__ double gfw_rs_score(const double *m, int cap, int n, int lane, double k, const double *t) {
    double acc = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double x2 = gfw_rs_residual2(k, m[i], m[cap + i], m[2 * cap + i], t);
        acc = acc + (x2 / (1.0 + x2));
    }
    return gfw_rs_wave_sum(acc);
}
// the six sums of w_i m_i m_i^T (w = 1 without `weighted`) -> the smallest eigenvector
__device__ __forceinline__ void gfw_rs_fit(const double *m, int cap, int n, int lane, double k, bool weighted, int sweeps, double *t) {
    double G[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < n; i += 64) {
        const double m0 = m[i], m1 = m[cap + i], m2 = m[2 * cap + i];
        if (weighted) {
            const double x2 = gfw_rs_residual2(k, m0, m1, m2, t);
            const double w = 1.0 / ((1.0 + x2) * (1.0 + x2));
            G[0] = G[0] + (w * (m0 * m0)); G[1] = G[1] + (w * (m0 * m1)); G[2] = G[2] + (w * (m0 * m2));
            G[3] = G[3] + (w * (m1 * m1)); G[4] = G[4] + (w * (m1 * m2)); G[5] = G[5] + (w * (m2 * m2));
        } else {
            G[0] = G[0] + (m0 * m0); G[1] = G[1] + (m0 * m1); G[2] = G[2] + (m0 * m2);
            G[3] = G[3] + (m1 * m1); G[4] = G[4] + (m1 * m2); G[5] = G[5] + (m2 * m2);
        }
    }
    #pragma unroll
    for (int j = 0; j < 6; ++j) G[j] = gfw_rs_wave_sum(G[j]);
    gfw_rs_smallest(G, sweeps, t);
}

// Cost stage: candidate blockIdx.x of pair blockIdx.y, one wave (workgroups of four waves, a candidate each, were measured beside it: no faster)
__global__ __launch_bounds__(64) void gfw_rs_cost_kernel(const GfwRsArgs A) {
    GFW_RS_DYN_LDS(s_m);                                                             // [3][lds_points]
    const int pair = (int)blockIdx.y, c = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int r = A.pair_range[pair];
    if (c >= gfw_rs_cand_count(A, r)) return;                                        // workgroup-uniform
    const int first = A.pair_first[pair], n = A.pair_first[pair + 1] - first, cap = A.lds_points;
    double cost = 0.0;
    if (n > 0) {                                                                     // workgroup-uniform
        const double d = gfw_rs_candidate(A, r, c);
        // the window of the lookups: the segments of the pair's earliest and latest point time at this delay (x + d is monotonic in x: every point's time lies between)
        double tmin = A.prep[(size_t)first * 4 + 3], tmax = tmin;
        for (int i = lane; i < n; i += 64) {
            const double ta = A.prep[(size_t)(first + i) * 4 + 3], tb = A.prep[((size_t)A.total + first + i) * 4 + 3];
            tmin = ta < tmin ? ta : tmin; tmin = tb < tmin ? tb : tmin;
            tmax = ta > tmax ? ta : tmax; tmax = tb > tmax ? tb : tmax;
        }
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double lo = __shfl_xor(tmin, off), hi = __shfl_xor(tmax, off);
            tmin = lo < tmin ? lo : tmin; tmax = hi > tmax ? hi : tmax;
        }
        const int wlo = gfw_rs_segment(A.track_t, 0, A.n_track - 1, gfw_rs_clamp(A.track_t, A.n_track, tmin + d));
        const int whi = gfw_rs_segment(A.track_t, 0, A.n_track - 1, gfw_rs_clamp(A.track_t, A.n_track, tmax + d)) + 1;
        for (int i = lane; i < n; i += 64) {
            double m[3];
            gfw_rs_moment_vector(A.track_t, A.track_q, A.n_track, wlo, whi, A.prep + (size_t)(first + i) * 4, A.prep + ((size_t)A.total + first + i) * 4, d, m);
            s_m[i] = m[0]; s_m[cap + i] = m[1]; s_m[2 * cap + i] = m[2];
        }
        __syncthreads();
        double t[3];
        gfw_rs_fit(s_m, cap, n, lane, A.loss_scale, false, A.sweeps, t);
        double best = gfw_rs_score(s_m, cap, n, lane, A.loss_scale, t);
        if (n >= 2) {
            for (int h = 1; h <= A.hypotheses; ++h) {
                const int i = (7 * h) % n, j = (13 * h + 5) % n;
                const double a[3] = {s_m[i], s_m[cap + i], s_m[2 * cap + i]}, b[3] = {s_m[j], s_m[cap + j], s_m[2 * cap + j]};
                double x[3];
                gfw_pe_cross(a, b, x);
                const double len2 = ((x[0] * x[0]) + (x[1] * x[1])) + (x[2] * x[2]);
                if (!(len2 > 0.0)) continue;                                         // wave-uniform: every lane holds the same m_i, m_j
                const double len = __builtin_sqrt(len2);
                const double th[3] = {x[0] / len, x[1] / len, x[2] / len};
                const double s = gfw_rs_score(s_m, cap, n, lane, A.loss_scale, th);
                if (s < best) { best = s; t[0] = th[0]; t[1] = th[1]; t[2] = th[2]; }
            }
        }
        for (int k = 0; k < A.refits; ++k) gfw_rs_fit(s_m, cap, n, lane, A.loss_scale, true, A.sweeps, t);
        cost = gfw_rs_score(s_m, cap, n, lane, A.loss_scale, t);
    }
    if (lane == 0) A.pair_costs[(A.mode == 0 ? (size_t)A.pc_first[pair] : (size_t)pair * A.n_cand) + c] = cost;
}

// Pick stage: workgroup blockIdx.x is a range.  A lane adds the pairs of a contiguous run of candidates and keeps the run's first minimum, lane 0 folds the lanes'
// picks in lane order: together the first minimum over the candidates in index order.  A NaN sum is never picked while another sum of the round is not NaN: a run
// takes only sums that are not NaN, a lane whose run held none is skipped like an empty one, and a round of nothing but NaN picks candidate 0 with its NaN cost.
__global__ __launch_bounds__(GFW_RS_LANES) void gfw_rs_pick_kernel(const GfwRsArgs A) {
    __shared__ double s_cost[GFW_RS_LANES];
    __shared__ int s_idx[GFW_RS_LANES];
    __shared__ int s_pick;
    __shared__ double s_centre;
    const int r = (int)blockIdx.x;
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int p0 = A.range_first[r], p1 = A.range_first[r + 1];
    const int n = gfw_rs_cand_count(A, r);
    double *sums = A.mode == 0 ? A.sums_all + A.cand_first[r] : A.sums_all + (size_t)r * A.total_cand + A.at;
    double *cands = A.mode == 0 ? nullptr : A.cand_all + (size_t)r * A.total_cand + A.at;
    if (A.mode != 0 && p1 == p0) {                                                   // workgroup-uniform: a range without pairs finds nothing
        if (A.mode == 1) {
            for (int i = t; i < A.total_cand; i += GFW_RS_LANES) { cands[i] = 0.0; sums[i] = 0.0; }
            if (t == 0) { gfw_sync_result o; o.found = 0; o.n_coarse = n; o.coarse_value = 0.0; o.coarse_cost = 0.0; o.value = 0.0; o.cost = 0.0; A.results[r] = o; }
        }
        return;
    }
    const int run = (n + GFW_RS_LANES - 1) / GFW_RS_LANES;
    const int c0 = t * run < n ? t * run : n, c1 = c0 + run < n ? c0 + run : n;
    double best = 0.0;
    int idx = -1;
    for (int c = c0; c < c1; ++c) {
        double sum = 0.0;
        for (int p = p0; p < p1; ++p) sum = sum + A.pair_costs[(A.mode == 0 ? (size_t)A.pc_first[p] : (size_t)p * A.n_cand) + c];
        sums[c] = sum;
        if (A.mode == 1) cands[c] = gfw_rs_candidate(A, r, c);
        if (sum == sum && (idx < 0 || sum < best)) { best = sum; idx = c; }         // a NaN sum is never taken: idx stays -1 where the whole run is NaN
    }
    if (A.mode == 0) return;                                                         // workgroup-uniform
    s_cost[t] = best; s_idx[t] = idx;
    __syncthreads();
    if (t == 0) {
        int pick = -1;
        double low = 0.0;
        for (int j = 0; j < GFW_RS_LANES; ++j) {
            if (s_idx[j] < 0) continue;
            if (pick < 0 || s_cost[j] < low) { low = s_cost[j]; pick = s_idx[j]; }
        }
        if (pick < 0) { pick = 0; low = sums[0]; }                                   // every sum of the round is NaN: candidate 0, its cost NaN (sums[0] is this lane's own store)
        const double centre = gfw_rs_candidate(A, r, pick);
        s_pick = pick; s_centre = centre;
        gfw_sync_result *res = A.results + r;
        if (A.mode == 1) { gfw_sync_result o; o.found = 1; o.n_coarse = n; o.coarse_value = centre; o.coarse_cost = low; o.value = 0.0; o.cost = 0.0; *res = o; }
        if (A.last) {
            double value = centre;
            if (A.refine && pick > 0 && pick < n - 1) {                              // (the sums of the neighbours are this workgroup's own stores, behind the barrier)
                const double ym = sums[pick - 1], yp = sums[pick + 1];
                const double den = (ym - (2.0 * low)) + yp;
                if (den > 0.0) value = centre + (A.step * ((0.5 * (ym - yp)) / den));
            }
            res->value = value; res->cost = low;
        }
    }
    __syncthreads();
    if (!A.last && t < GFW_RS_LATER) cands[n + t] = s_centre + ((double)(t - 8) * A.next_step);
}

#ifndef GFW_HOST_INTERPRETER                                                         // (the interpreter is its own launcher)
hipError_t gfw_launch_rs_prepare(const gfw_kernel_params &P, const GfwCommon &C, const GfwRsArgs &A, hipStream_t s) {
    if (A.total <= 0) return hipSuccess;
    const dim3 grid((unsigned)((2 * (size_t)A.total + GFW_RS_LANES - 1) / GFW_RS_LANES));
    if (C.model == GFW_MODEL_OPENCV_FISHEYE) hipLaunchKernelGGL(gfw_rs_prepare_kernel<GFW_MODEL_OPENCV_FISHEYE>, grid, dim3(64, 4), 0, s, P, C, A);
    else hipLaunchKernelGGL(gfw_rs_prepare_kernel<-1>, grid, dim3(64, 4), 0, s, P, C, A);
    return hipGetLastError();
}
hipError_t gfw_launch_rs_costs(const GfwRsArgs &A, int max_candidates, hipStream_t s) {
    if (A.n_pairs <= 0 || max_candidates <= 0) return hipSuccess;
    const size_t lds = sizeof(double) * 3 * (size_t)A.lds_points;
    if (lds > 48 * 1024) {                                                           // above the default limit of dynamic LDS a kernel has to be told
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gfw_rs_cost_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gfw_rs_cost_kernel, dim3((unsigned)max_candidates, (unsigned)A.n_pairs), dim3(64), lds, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_rs_pick(const GfwRsArgs &A, hipStream_t s) {
    if (A.n_ranges <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_rs_pick_kernel, dim3((unsigned)A.n_ranges), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
#endif
