// gfw_sync.h — the visual-features offset / readout-time search on the device (gfw_sync.hip): calculate_distance of
// find_offset/visual_features.rs:49-83 for every candidate of a range, and the two-stage search of :87-131
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_matrices.h"

#define GFW_SYNC_LANES 64           // lanes of a (candidate, pair) workgroup: one wave
#define GFW_SYNC_PAIR_MAX 4096      // points of one pair: their u32 distances fill the 16 KB of LDS the cost kernel may ask for
#define GFW_SYNC_FINE 200           // candidates of the second stage (:99, :123)
#define GFW_SYNC_REDUCE_LANES 256   // lanes of the one workgroup that sums a stage's partials and picks its minimum
#define GFW_SYNC_PAIRS_MAX 65535    // pairs ride on blockIdx.y

struct GfwSyncArgs {
    GfwTracks T;                    // the context's tracks; off_n = 0 when the search clears the sync offsets (:13-15)
    gfw_zoom_frame F;               // new_k and video_rotation_deg, in the form gfw_zoom_rotation reads (suppress_rotation 0)
    const int64_t *pair_ts;         // [n_pairs][2] timestamps_us of a pair's two frames (device)
    const int32_t *pair_first;      // [n_pairs + 1] first point of each pair (device)
    const float *points;            // [2][total][2]: every pair's points of the first frame, then of the second (device)
    float4 *rays;                   // [2][total]: the lens stage's (ptx, pty, ok, 0) per point (device)
    const double *candidates;       // [n][2] (offset_ms, frame_readout_time_ms) (device)
    unsigned long long *partial;    // [n][n_pairs]: a pair's contribution to a candidate's cost (device)
    float *mapped;                  // nullptr or [n][total][2][2]: p1, p2 as mapped (device)
    const gfw_sync_result *gate;    // nullptr, or the search's result: a stage behind a search that found nothing does nothing
    float w, h;                     // `w as f32`, `h as f32` of the bounds test
    int32_t horizontal, readout_dim, n_pairs, total;
};
struct GfwSyncReduceArgs {
    const unsigned long long *partial;   // [n][n_pairs]
    const double *candidates;            // [n][2]
    double *costs;                       // nullptr or [n]
    gfw_sync_result *result;             // nullptr: costs only
    double *fine;                        // stage 0: the [200][2] candidates of the second stage, written from the pick
    int32_t n, n_pairs, column, stage;   // column: which entry of a candidate the search varies (0 offset, 1 readout time); stage 0 coarse, 1 fine
};
// the lens stage of 2 * total points; `n` candidates x n_pairs pairs; one workgroup.  Zero-sized launches are skipped.
hipError_t gfw_launch_sync_rays(const gfw_kernel_params &P, const GfwCommon &C, const GfwSyncArgs &A, hipStream_t s);
hipError_t gfw_launch_sync_costs(const GfwSyncArgs &A, int n, int max_pair_points, hipStream_t s);
hipError_t gfw_launch_sync_reduce(const GfwSyncReduceArgs &R, hipStream_t s);
