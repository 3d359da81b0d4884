// gfw_sync_gyro.h — the gyro-match offset search on the device (gfw_sync_gyro.hip): calculate_cost of find_offset/essential_matrix.rs:109-131 for every candidate of
// every range, and the two-stage search of :52-75
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gfwarp.h"

#define GFW_GYRO_LANES 256              // lanes of a workgroup of either kernel: a lane of the cost kernel is a candidate
#define GFW_GYRO_FINE 200               // candidates of the second stage (:66)
#define GFW_GYRO_RANGES_MAX 65535       // ranges ride on blockIdx.y
#define GFW_GYRO_EST_MAX 65536          // estimated samples of a range
#define GFW_GYRO_SAMPLES_MAX (1 << 22)  // gyro samples of a range
#define GFW_GYRO_COARSE_MAX 2000000     // coarse candidates of a range (search_size_ms up to 10^6), or caller-given candidates of a range

// `v as usize` of a double (Rust: truncating, saturating, NaN -> 0), written out: a plain conversion of an out-of-range double is undefined
__host__ __device__ inline unsigned long long gfw_gyro_key(double v) {
    if (!(v >= 1.0)) return 0ull;                                  // NaN, negatives, [0, 1)
    if (v >= 18446744073709551616.0) return 0xffffffffffffffffull;
    return (unsigned long long)v;
}

// One range as staged: its slices of the arrays below.  The gyro slice is the BTreeMap of :50 flattened — keys ascending, one entry per key.
struct GfwGyroRange { long long est_first, gyro_first, cand_first; int32_t est_n, gyro_n, cand_n, pad; };

struct GfwGyroArgs {
    const GfwGyroRange *ranges;         // [n_ranges] (device)
    const double *est;                  // [][4] (timestamp_ms, x, y, z) of every estimated sample (device)
    const uint8_t *est_has;             // [] 0 = `gyro: None`
    const unsigned long long *keys;     // [] `(timestamp_ms * 1000.0) as usize` of every gyro entry
    const double *gyro;                 // [][4] (x, y, z, 1.0 or — `gyro: None` — 0.0) of every gyro entry
    const double *candidates;           // stage 0: every range's candidate offsets, at its cand_first; stage 1: [n_ranges][200], written by the pick kernel
    double *costs;                      // laid out as the candidates are
    const gfw_sync_result *gate;        // stage 1: [n_ranges]; a range that found nothing has no second stage
    int32_t stage, pad;
};
struct GfwGyroPickArgs {
    const GfwGyroRange *ranges;
    const double *candidates;           // as GfwGyroArgs
    const double *costs;
    gfw_sync_result *results;           // [n_ranges]
    double *fine;                       // stage 0: [n_ranges][200], the candidates of the second stage
    double *fine_costs;                 // stage 1: nullptr or the caller's [n_ranges][200], zeroed for a range that found nothing
    int32_t stage, pad;
};
// `max_candidates`: the largest cand_n of the call (stage 1: 200).  Zero-sized launches are skipped.
hipError_t gfw_launch_gyro_costs(const GfwGyroArgs &A, int n_ranges, int max_candidates, hipStream_t s);
hipError_t gfw_launch_gyro_pick(const GfwGyroPickArgs &R, int n_ranges, hipStream_t s);
