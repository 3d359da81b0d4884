// gfw_sync_gyro.hip — the gyro-match offset search (src/core/synchronization/find_offset/essential_matrix.rs:13-131; offset method 0 and the fast initial offset of rs-sync).
//
// The reference evaluates calculate_cost (:109-131) for `search_size as usize * 2` coarse and 200 fine candidate offsets of a range under rayon on the host: per
// candidate every estimated sample is looked up in a BTreeMap of the gyro samples keyed by integer microseconds (the first key at or above the query) and the
// weighted squared differences of the matches are averaged.  Candidates and ranges are independent and the arithmetic is f64, so here a lane is a candidate:
// it walks its range's estimated samples in index order — the reference's own fold, three separate additions per match — and bisects the range's sorted key array
// per sample.  The samples of a range are the same for all lanes (uniform loads); neighbouring lanes are candidates 1 ms (or 0.01 ms) apart, so their hits are
// neighbouring gyro entries.  A pick kernel, one workgroup per range, folds the costs the way `reduce_with(find_min)` does — `if a.1 < b.1 { a } else { b }` left to
// right: the LAST minimal candidate — and behind the coarse stage writes the 200 fine candidates for the next cost launch.  Plain C++ under -ffp-contract=off;
// all stores are ordinary vector stores; the one barrier sits in workgroup-uniform control flow.
#include <hip/hip_runtime.h>
#include "gfw_sync_gyro.h"

#define GFW_GYRO_F64_MAX 1.7976931348623157e308                                      // f64::MAX (:129)

// calculate_cost of one candidate (:109-131)
__device__ __forceinline__ double gfw_gyro_cost(const GfwGyroArgs &A, const GfwGyroRange &G, double offs) {
    const double *est = A.est + G.est_first * 4;
    const uint8_t *est_has = A.est_has + G.est_first;
    const unsigned long long *keys = A.keys + G.gyro_first;
    const double *gyro = A.gyro + G.gyro_first * 4;
    double sum = 0.0;
    int matches = 0;
    for (int j = 0; j < G.est_n; ++j) {
        const unsigned long long q = gfw_gyro_key((est[(size_t)j * 4] - offs) * 1000.0);      // gyro_at_timestamp(o.timestamp_ms - offs): `(ts * 1000.0) as usize` (:106)
        int lo = 0, hi = G.gyro_n;                                                   // range(q..).next(): the first key at or above the query
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (keys[mid] < q) lo = mid + 1; else hi = mid;
        }
        if (lo >= G.gyro_n) continue;                                                // past the last key: a miss
        const double *g = gyro + (size_t)lo * 4;
        if (g[3] == 0.0 || !est_has[j]) continue;                                    // a None on either side is no match, and nothing further is looked at
        const double *o = est + (size_t)j * 4 + 1;
        const double d0 = g[0] - o[0], d1 = g[1] - o[1], d2 = g[2] - o[2];
        matches += 1;
        sum += (d0 * d0) * 70.0;                                                     // :117-119, `powi(2)` = x * x
        sum += (d1 * d1) * 70.0;
        sum += (d2 * d2) * 100.0;
    }
    if (G.est_n > 0 && matches > G.est_n / 2) return sum / (double)matches;          // :124-126
    return GFW_GYRO_F64_MAX;
}

// Cost stage: candidate blockIdx.x * 256 + lane, range blockIdx.y
__global__ __launch_bounds__(GFW_GYRO_LANES) void gfw_gyro_cost_kernel(const GfwGyroArgs A) {
    const int r = (int)blockIdx.y;
    const int c = (int)(blockIdx.x * (unsigned)GFW_GYRO_LANES + threadIdx.y * 64u + threadIdx.x);
    const GfwGyroRange G = A.ranges[r];
    const int n = A.stage ? GFW_GYRO_FINE : G.cand_n;
    if (c >= n) return;
    if (A.stage && !A.gate[r].found) return;
    const size_t at = (A.stage ? (size_t)r * GFW_GYRO_FINE : (size_t)G.cand_first) + (size_t)c;
    A.costs[at] = gfw_gyro_cost(A, G, A.candidates[at]);
}

// Pick stage: workgroup blockIdx.x is a range.  A lane folds a contiguous run of candidates, lane 0 folds the lanes' picks in lane order: together the left fold of
// find_min over the candidates in index order.
__global__ __launch_bounds__(GFW_GYRO_LANES) void gfw_gyro_pick_kernel(const GfwGyroPickArgs R) {
    __shared__ double s_cost[GFW_GYRO_LANES];
    __shared__ int s_idx[GFW_GYRO_LANES];
    __shared__ int s_pick;
    const int r = (int)blockIdx.x;
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const GfwGyroRange G = R.ranges[r];
    gfw_sync_result *res = R.results + r;
    if (R.stage == 1 && !res->found) {                                               // workgroup-uniform: a search without candidates has no second stage
        if (R.fine_costs && t < GFW_GYRO_FINE) R.fine_costs[(size_t)r * GFW_GYRO_FINE + t] = 0.0;
        return;
    }
    const int n = R.stage ? GFW_GYRO_FINE : G.cand_n;
    const size_t base = R.stage ? (size_t)r * GFW_GYRO_FINE : (size_t)G.cand_first;
    const int run = (n + GFW_GYRO_LANES - 1) / GFW_GYRO_LANES;
    const int c0 = t * run < n ? t * run : n, c1 = c0 + run < n ? c0 + run : n;
    double best = 0.0;
    int idx = -1;
    for (int c = c0; c < c1; ++c) {
        const double cost = R.costs[base + c];
        if (idx < 0 || !(best < cost)) { best = cost; idx = c; }                     // `if a.1 < b.1 { a } else { b }`
    }
    s_cost[t] = best; s_idx[t] = idx;
    __syncthreads();
    if (t == 0) {
        int pick = -1;
        double low = 0.0;
        for (int j = 0; j < GFW_GYRO_LANES; ++j) {
            if (s_idx[j] < 0) continue;
            if (pick < 0 || !(low < s_cost[j])) { low = s_cost[j]; pick = s_idx[j]; }
        }
        s_pick = pick;
        const double value = pick >= 0 ? R.candidates[base + pick] : 0.0;
        if (R.stage == 0) {
            gfw_sync_result o;
            o.found = pick >= 0 ? 1 : 0; o.n_coarse = n;
            o.coarse_value = value; o.coarse_cost = low; o.value = 0.0; o.cost = 0.0;
            *res = o;
        } else if (pick >= 0) { res->value = value; res->cost = low; }
    }
    __syncthreads();
    if (R.stage == 0 && s_pick >= 0 && t < GFW_GYRO_FINE) {
        const double lowest = R.candidates[base + s_pick];
        const double step = 2.0 / 200.0;                                             // :65-67
        R.fine[(size_t)r * GFW_GYRO_FINE + t] = lowest + (-2.0 + ((double)t * step)); // :71 — below the coarse pick only
    }
}

hipError_t gfw_launch_gyro_costs(const GfwGyroArgs &A, int n_ranges, int max_candidates, hipStream_t s) {
    if (n_ranges <= 0 || max_candidates <= 0) return hipSuccess;
    const dim3 grid((unsigned)((max_candidates + GFW_GYRO_LANES - 1) / GFW_GYRO_LANES), (unsigned)n_ranges);
    hipLaunchKernelGGL(gfw_gyro_cost_kernel, grid, dim3(64, GFW_GYRO_LANES / 64), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_gyro_pick(const GfwGyroPickArgs &R, int n_ranges, hipStream_t s) {
    if (n_ranges <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_gyro_pick_kernel, dim3((unsigned)n_ranges), dim3(64, GFW_GYRO_LANES / 64), 0, s, R);
    return hipGetLastError();
}
