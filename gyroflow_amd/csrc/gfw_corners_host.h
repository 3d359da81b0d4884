// gfw_corners_host.h — host only: what gfw_corners_shi_tomasi checks, sizes and stages for the kernels of gfw_corners.hip.  Included behind gfw_corners.h
// (GfwCornersArgs) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "gfw_layout.h"

// The caller's arguments of one call (include/gfwarp.h: gfw_corners_shi_tomasi)
struct GfwCornersInputs {
    int width, height, stride, max_corners; float quality, min_distance; int max_workspace_mb, reserved;
    const void *frames; int frames_on_device, n_frames;
    const void *corners, *counts, *feat_first, *features;       // only asked whether they are there
};

// What a call with frames needs.  A frame's candidate list has room for EVERY interior pixel (8 B each: a plateau image makes all of them candidates), so the
// frames are dealt into batches whose lists fit max_workspace_mb (0: 512); each batch is two launches.  The staged block: [n_frames] frame maxima and [n_frames]
// candidate counts (zeros: the upload clears what the kernels fold into), then the frames where they are host memory.
struct GfwCornersPlan {
    int64_t slots; size_t list_bytes, workspace_cap;            // of one frame; the bytes the lists of a batch may take
    int batch_frames, n_batches;                                // frames of a full batch (the last one has the rest)
    int tiles_x, tiles_y;
    size_t frame_bytes, cand_bytes;                             // cand_bytes: the lists of a full batch
    size_t o_max, o_count, o_frames, total;
};
inline GfwCornersPlan gfw_corners_plan(const GfwCornersInputs &I) {
    GfwCornersPlan P;
    memset(&P, 0, sizeof(P));
    P.slots = (int64_t)(I.width - 2) * (int64_t)(I.height - 2);
    P.list_bytes = sizeof(uint64_t) * (size_t)P.slots;
    P.workspace_cap = (size_t)(I.max_workspace_mb > 0 ? I.max_workspace_mb : GFW_CORNERS_WORKSPACE_MB) << 20;
    const size_t fit = P.workspace_cap / P.list_bytes;
    P.batch_frames = fit < (size_t)I.n_frames ? (int)fit : I.n_frames;
    P.n_batches = P.batch_frames > 0 ? (I.n_frames + P.batch_frames - 1) / P.batch_frames : 0;
    P.tiles_x = (I.width + GFW_CORNERS_TILE_W - 1) / GFW_CORNERS_TILE_W; P.tiles_y = (I.height + GFW_CORNERS_TILE_H - 1) / GFW_CORNERS_TILE_H;
    P.frame_bytes = (size_t)I.stride * (size_t)I.height;
    P.cand_bytes = P.list_bytes * (size_t)P.batch_frames;
    BlockLayout L;
    P.o_max = L.add(sizeof(uint32_t) * (size_t)I.n_frames);
    P.o_count = L.add(sizeof(uint32_t) * (size_t)I.n_frames);
    P.o_frames = L.add(I.frames_on_device ? 0 : P.frame_bytes * (size_t)I.n_frames);
    P.total = L.total;
    return P;
}
// -> true, or false with the reason in `err`
inline bool gfw_corners_check(const GfwCornersInputs &I, char *err, size_t cap) {
    if (I.reserved) { snprintf(err, cap, "bad corners configuration: the reserved slot must be 0"); return false; }
    if (I.n_frames < 0) { snprintf(err, cap, "bad corners arguments (negative count: %d frames)", I.n_frames); return false; }
    if (I.width < GFW_CORNERS_SIDE_MIN || I.width > GFW_CORNERS_SIDE_MAX || I.height < GFW_CORNERS_SIDE_MIN || I.height > GFW_CORNERS_SIDE_MAX) {
        snprintf(err, cap, "bad corners configuration: frames of %d x %d, both sides must be between %d and %d", I.width, I.height, GFW_CORNERS_SIDE_MIN, GFW_CORNERS_SIDE_MAX); return false; }
    if (I.stride < I.width) { snprintf(err, cap, "bad corners configuration: stride %d under the width %d", I.stride, I.width); return false; }
    if (I.max_corners < 1 || I.max_corners > GFW_CORNERS_MAX) { snprintf(err, cap, "bad corners configuration: max_corners %d, must be between 1 and %d", I.max_corners, GFW_CORNERS_MAX); return false; }
    if (!(I.quality > 0.0f && I.quality <= 1.0f)) { snprintf(err, cap, "bad corners configuration: quality %g, must be finite in (0, 1]", (double)I.quality); return false; }      // (false for a NaN)
    if (!(I.min_distance >= 0.0f && I.min_distance <= GFW_CORNERS_DISTANCE_MAX)) {
        snprintf(err, cap, "bad corners configuration: min_distance %g, must be finite in [0, %g]", (double)I.min_distance, (double)GFW_CORNERS_DISTANCE_MAX); return false; }
    if (I.max_workspace_mb < 0) { snprintf(err, cap, "bad corners configuration: max_workspace_mb %d is negative (0 = %d)", I.max_workspace_mb, GFW_CORNERS_WORKSPACE_MB); return false; }
    if (I.n_frames > GFW_CORNERS_FRAMES_MAX) { snprintf(err, cap, "%d frames: at most %d in a call", I.n_frames, GFW_CORNERS_FRAMES_MAX); return false; }
    if (I.n_frames == 0) return true;
    if (!I.frames) { snprintf(err, cap, "bad corners arguments (%d frames without their planes)", I.n_frames); return false; }
    if (!I.corners || !I.counts) { snprintf(err, cap, "bad corners arguments (a null corners / counts array)"); return false; }
    if (!I.feat_first != !I.features) { snprintf(err, cap, "bad corners arguments (feat_first and features: both or neither)"); return false; }
    const GfwCornersPlan P = gfw_corners_plan(I);
    if (P.batch_frames < 1) {
        snprintf(err, cap, "max_workspace_mb %d is too small: the candidate list of ONE %d x %d frame needs %zu bytes (%zu MB)", I.max_workspace_mb, I.width, I.height, P.list_bytes,
                 (P.list_bytes + ((size_t)1 << 20) - 1) >> 20); return false; }
    if (P.total > GFW_CORNERS_STAGED_MAX) {
        snprintf(err, cap, "the call stages %zu bytes (%d frames of stride %d x %d rows): at most 2 GiB", P.total, I.frames_on_device ? 0 : I.n_frames, I.stride, I.height); return false; }
    return true;
}

// Fills the block at (h, d) and everything of the argument block that does not change between the batches; the lists are at `cand` (device)
inline void gfw_corners_fill(const GfwCornersPlan &P, const GfwCornersInputs &I, char *h, char *d, unsigned long long *cand, GfwCornersArgs &A) {
    memset(h + P.o_max, 0, sizeof(uint32_t) * (size_t)I.n_frames);
    memset(h + P.o_count, 0, sizeof(uint32_t) * (size_t)I.n_frames);
    const uint8_t *frames = (const uint8_t *)I.frames;
    if (!I.frames_on_device) {
        memcpy(h + P.o_frames, I.frames, P.frame_bytes * (size_t)I.n_frames);
        frames = (const uint8_t *)(d + P.o_frames);
    }
    A.frames = frames; A.frame_bytes = (int64_t)P.frame_bytes;
    A.w = I.width; A.h = I.height; A.stride = I.stride; A.n_frames = I.n_frames;
    A.max_corners = I.max_corners; A.quality = I.quality; A.min_distance = I.min_distance;
    A.frame0 = 0; A.batch_frames = 0;
    A.tiles_x = P.tiles_x; A.tiles_y = P.tiles_y;
    A.slots = P.slots; A.cand = cand;
    A.max_bits = (uint32_t *)(d + P.o_max); A.cand_count = (uint32_t *)(d + P.o_count);
}
// Batch b of the plan: its first frame and its frames
inline void gfw_corners_batch(const GfwCornersPlan &P, int b, GfwCornersArgs &A) {
    A.frame0 = b * P.batch_frames;
    A.batch_frames = A.n_frames - A.frame0 < P.batch_frames ? A.n_frames - A.frame0 : P.batch_frames;
}
