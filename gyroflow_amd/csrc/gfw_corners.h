// gfw_corners.h — Shi-Tomasi corner detection of a clip's frames on the device (gfw_corners.hip): what `OFOpenCVPyrLK::detect_features`
// (src/core/synchronization/optical_flow/opencv_pyrlk.rs:25-42) asks of good_features_to_track(img, 200, 0.01, 10.0, no mask, blockSize 3, useHarris false, 0.04),
// stated with every sum an integer (tests/_cornerstmt.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GFW_CORNERS_TILE_W 64           // output pixels of a workgroup: 64 x 16, four rows a lane
#define GFW_CORNERS_TILE_H 16
#define GFW_CORNERS_SIDE_MIN 3          // one interior pixel
#define GFW_CORNERS_SIDE_MAX 8192
#define GFW_CORNERS_MAX 4096            // corners of a frame: gfw_flow_pyrlk's features-a-frame limit
#define GFW_CORNERS_FRAMES_MAX 4096
#define GFW_CORNERS_DISTANCE_MAX 1024.0f
#define GFW_CORNERS_WORKSPACE_MB 512    // the default of max_workspace_mb: room for one frame of 8192 x 8192 (8190^2 * 8 B < 512 MiB)
#define GFW_CORNERS_STAGED_MAX ((size_t)1 << 31)       // bytes of one staged block (the counters, host frames)

struct GfwCornersArgs {
    const uint8_t *frames; int64_t frame_bytes;        // frame f: frames + f * frame_bytes
    int32_t w, h, stride, n_frames;
    int32_t max_corners; float quality, min_distance;
    int32_t frame0, batch_frames;       // the frames of this batch: frame0 .. frame0 + batch_frames - 1
    int32_t tiles_x, tiles_y;
    int64_t slots;                      // candidate slots of a frame: every interior pixel, (w - 2) * (h - 2) — a list cannot overflow
    unsigned long long *cand;           // [batch_frames][slots] keys bits(e) << 32 | (y << 13 | x) in arbitrary order; 0 = killed (a key is never 0: e > 0)
    uint32_t *max_bits;                 // [n_frames] bits of max(e, 0) over the frame, zero before the eig launch (in the staged block: the upload clears it)
    uint32_t *cand_count;               // [n_frames] likewise
    float *corners;                     // [n_frames][max_corners][2]
    float *scores;                      // nullptr, or [n_frames][max_corners]
    int32_t *counts;                    // [n_frames]
    int32_t *feat_first;                // nullptr, or [n_frames + 1]
    float *features;                    // with feat_first: [kept][2]
};

// Two launches per batch (every tile of every frame of the batch; a workgroup per frame), then two for the packed form where it is asked for.
// Zero-sized launches are skipped.
hipError_t gfw_launch_corners_eig(const GfwCornersArgs &A, hipStream_t s);
hipError_t gfw_launch_corners_pick(const GfwCornersArgs &A, hipStream_t s);
hipError_t gfw_launch_corners_scan(const GfwCornersArgs &A, hipStream_t s);
hipError_t gfw_launch_corners_pack(const GfwCornersArgs &A, hipStream_t s);
