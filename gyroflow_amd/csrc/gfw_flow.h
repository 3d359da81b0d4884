// gfw_flow.h — pyramidal Lucas-Kanade optical flow of a clip's frame pairs on the device (gfw_flow.hip): what `OFOpenCVPyrLK::optical_flow_to`
// (src/core/synchronization/optical_flow/opencv_pyrlk.rs:63-119) asks of calcOpticalFlowPyrLK (window 21 x 21, maxLevel 3, 30 iterations or eps 0.01, flags 0,
// minEigThreshold 1e-4), stated in fixed point (tests/_flowstmt.py), and the grid points with their texture-variance filter of opencv_dis.rs:62-119.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GFW_FLOW_WIN 21             // the window's side
#define GFW_FLOW_HALF 10            // (WIN - 1) / 2
#define GFW_FLOW_WIN_PIXELS 441
#define GFW_FLOW_LANE_PIXELS 7      // window pixels of a lane: pixel k = lane + 64 m, m < 7 (448 >= 441)
#define GFW_FLOW_LEVELS 4           // maxLevel 3
#define GFW_FLOW_ITERS 30
#define GFW_FLOW_SIDE_MIN 24        // a level's smallest side (gfw_flow.hip has the proof); also the smallest frame
#define GFW_FLOW_SIDE_MAX 8192
#define GFW_FLOW_FEATURES_MAX 4096  // features of a frame (grid nodes in the grid mode)
#define GFW_FLOW_PAIRS_MAX 65535    // pairs ride on blockIdx.y
#define GFW_FLOW_FRAMES_MAX 4096    // frames ride on blockIdx.y of the pyramid launches
#define GFW_FLOW_STAGED_MAX ((size_t)1 << 31)      // bytes of one staged block (pairs, features, host frames)
#define GFW_FLOW_MODE_FEATURES 0
#define GFW_FLOW_MODE_GRID 1

struct GfwFlowLevel { const uint8_t *base; int64_t frame_bytes; int32_t w, h, stride, pad_; };      // frame f of the level: base + f * frame_bytes
struct GfwFlowArgs {
    GfwFlowLevel lv[GFW_FLOW_LEVELS];   // [0] the caller's frames, [1 .. top] work space (stride = w)
    const int32_t *pair_frames;     // [n_pairs][2] (device)
    const int32_t *raw_first;       // [n_pairs + 1] first raw slot of each pair (device)
    const int32_t *feat_first;      // mode 0: [n_frames + 1] (device)
    const float *features;          // mode 0: [total][2] (device)
    float *grid_points;             // mode 1: [n_frames][grid_nodes][2], the kept nodes of a frame first, in the reference's loop order
    int32_t *grid_counts;           // mode 1: [n_frames]
    float *next;                    // [raw][2]
    uint8_t *status;                // [raw]
    int32_t *iters;                 // nullptr, or [raw][4]
    int32_t *kept;                  // [n_pairs] kept points of each pair, zero before the tracker (in the staged block: the upload clears it)
    int32_t *out_pair_first;        // [n_pairs + 1]
    float *points_a, *points_b;     // [kept][2]
    int32_t top;                    // L: the coarsest level built
    int32_t n_frames, n_pairs, mode;
    int32_t max_features;           // the tracker's grid.x: the most features any pair of the call can have
    int32_t grid_step, grid_half, grid_rows, grid_nodes;      // mode 1: `step`, `half_win`, nodes of a column (the inner loop), nodes of a frame
};

// One launch per level 1 .. top (all frames); the grid points of every frame (mode 1); a wave per (pair, feature); the scan over the pairs; a workgroup per pair.
// Zero-sized launches are skipped.
hipError_t gfw_launch_flow_pyramid(const GfwFlowArgs &A, int level, uint8_t *dst, hipStream_t s);
hipError_t gfw_launch_flow_grid(const GfwFlowArgs &A, hipStream_t s);
hipError_t gfw_launch_flow_track(const GfwFlowArgs &A, hipStream_t s);
hipError_t gfw_launch_flow_scan(const GfwFlowArgs &A, hipStream_t s);
hipError_t gfw_launch_flow_compact(const GfwFlowArgs &A, hipStream_t s);
