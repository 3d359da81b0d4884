// gfw_flow_host.h — host only: what gfw_flow_pyrlk checks, sizes and stages for the kernels of gfw_flow.hip.  Included behind gfw_flow.h (GfwFlowArgs) by gfw_api.hip
// and by whatever else stages a call for those kernels; no kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "gfw_layout.h"

// The caller's arguments of one call (include/gfwarp.h: gfw_flow_pyrlk)
struct GfwFlowInputs {
    int width, height, stride, mode, reserved;
    const void *frames; int frames_on_device, n_frames;
    const int32_t *pair_frames; int n_pairs;
    const int32_t *feat_first; const float *features;
};

// The pyramid: the sides of level l + 1 are (w_l + 1) / 2 and (h_l + 1) / 2; levels 0 .. top are built, top the largest l <= 3 whose two sides are both >= 24
inline int gfw_flow_levels(int width, int height, int *lw, int *lh) {
    int top = 0;
    lw[0] = width; lh[0] = height;
    for (int l = 1; l < GFW_FLOW_LEVELS; ++l) {
        lw[l] = (lw[l - 1] + 1) / 2; lh[l] = (lh[l - 1] + 1) / 2;
        if (top == l - 1 && lw[l] >= GFW_FLOW_SIDE_MIN && lh[l] >= GFW_FLOW_SIDE_MIN) top = l;
    }
    return top;
}
// The grid of opencv_dis.rs:62-72: `step = w / 15`, `window_size = max(10, round(w * 0.02))` in f32 (half away from zero), `half_win = window_size / 2`;
// `(0..h).step_by(step)` has ceil(h / step) nodes
struct GfwFlowGrid { int step, half, rows, cols, nodes; };
inline GfwFlowGrid gfw_flow_grid(int width, int height) {
    GfwFlowGrid G;
    G.step = width / 15;                                     // >= 1: width >= 24
    int win = (int)roundf((float)width * 0.02f);
    if (win < 10) win = 10;
    G.half = win / 2;
    G.cols = (width + G.step - 1) / G.step; G.rows = (height + G.step - 1) / G.step;
    G.nodes = G.cols * G.rows;
    return G;
}

// What a call with pairs needs (its arrays checked as far as gfw_flow_check has come when it asks): the levels, the grid, the raw slots (every pair's features, or every node of the grid per pair), the staged block
// [n_pairs][2] frames, [n_pairs + 1] first raw slots, [n_pairs] kept counts (zeros: the upload clears what the tracker adds to), and in mode 0 [n_frames + 1] feature
// firsts (from 0) and the features; then the frames where they are host memory.
struct GfwFlowPlan {
    int top, lw[GFW_FLOW_LEVELS], lh[GFW_FLOW_LEVELS];
    GfwFlowGrid grid;
    int64_t raw_total; int max_features, n_features;
    size_t frame_bytes, level_at[GFW_FLOW_LEVELS], pyramid_bytes;            // the work space of levels 1 .. top ([n_frames][h_l][w_l] each)
    size_t o_pairs, o_raw, o_kept, o_ffirst, o_feat, o_frames, total;
};
inline GfwFlowPlan gfw_flow_plan(const GfwFlowInputs &I) {
    GfwFlowPlan P;
    memset(&P, 0, sizeof(P));
    P.top = gfw_flow_levels(I.width, I.height, P.lw, P.lh);
    P.grid = gfw_flow_grid(I.width, I.height);
    P.frame_bytes = (size_t)I.stride * (size_t)I.height;
    BlockLayout W;
    for (int l = 1; l <= P.top; ++l) P.level_at[l] = W.add((size_t)I.n_frames * (size_t)P.lw[l] * (size_t)P.lh[l]);
    P.pyramid_bytes = W.total;
    for (int p = 0; p < I.n_pairs; ++p) {
        const int a = I.pair_frames[p * 2];
        const int n = I.mode == GFW_FLOW_MODE_GRID ? P.grid.nodes : I.feat_first[a + 1] - I.feat_first[a];
        P.raw_total += n;
        if (n > P.max_features) P.max_features = n;
    }
    P.n_features = I.mode == GFW_FLOW_MODE_FEATURES && I.n_pairs ? I.feat_first[I.n_frames] - I.feat_first[0] : 0;
    BlockLayout L;
    P.o_pairs = L.add(sizeof(int32_t) * 2 * (size_t)I.n_pairs);
    P.o_raw = L.add(sizeof(int32_t) * ((size_t)I.n_pairs + 1));
    P.o_kept = L.add(sizeof(int32_t) * (size_t)I.n_pairs);
    P.o_ffirst = L.add(I.mode == GFW_FLOW_MODE_FEATURES ? sizeof(int32_t) * ((size_t)I.n_frames + 1) : 0);
    P.o_feat = L.add(sizeof(float) * 2 * (size_t)P.n_features);
    P.o_frames = L.add(I.frames_on_device ? 0 : P.frame_bytes * (size_t)I.n_frames);
    P.total = L.total;
    return P;
}
// -> true, or false with the reason (the pair or frame named) in `err`
inline bool gfw_flow_check(const GfwFlowInputs &I, char *err, size_t cap) {
    if (I.reserved) { snprintf(err, cap, "bad flow configuration: the reserved slot must be 0"); return false; }
    if (I.n_frames < 0 || I.n_pairs < 0) { snprintf(err, cap, "bad flow arguments (negative count: %d frames, %d pairs)", I.n_frames, I.n_pairs); return false; }
    if (I.width < GFW_FLOW_SIDE_MIN || I.width > GFW_FLOW_SIDE_MAX || I.height < GFW_FLOW_SIDE_MIN || I.height > GFW_FLOW_SIDE_MAX) {
        snprintf(err, cap, "bad flow configuration: frames of %d x %d, both sides must be between %d and %d", I.width, I.height, GFW_FLOW_SIDE_MIN, GFW_FLOW_SIDE_MAX); return false; }
    if (I.stride < I.width) { snprintf(err, cap, "bad flow configuration: stride %d under the width %d", I.stride, I.width); return false; }
    if (I.mode != GFW_FLOW_MODE_FEATURES && I.mode != GFW_FLOW_MODE_GRID) { snprintf(err, cap, "bad flow configuration: point mode %d (0 the caller's features, 1 the grid points)", I.mode); return false; }
    if (I.n_frames > GFW_FLOW_FRAMES_MAX) { snprintf(err, cap, "%d frames: at most %d in a call", I.n_frames, GFW_FLOW_FRAMES_MAX); return false; }
    if (I.n_pairs > GFW_FLOW_PAIRS_MAX) { snprintf(err, cap, "%d pairs: at most %d in a call", I.n_pairs, GFW_FLOW_PAIRS_MAX); return false; }
    if (I.n_pairs == 0) return true;
    if (!I.pair_frames) { snprintf(err, cap, "bad flow arguments (pairs without pair_frames)"); return false; }
    if (I.n_frames && !I.frames) { snprintf(err, cap, "bad flow arguments (%d frames without their planes)", I.n_frames); return false; }
    if (I.mode == GFW_FLOW_MODE_FEATURES) {
        if (!I.feat_first) { snprintf(err, cap, "bad flow arguments (point mode 0 without features: feat_first is null)"); return false; }
        if (I.feat_first[0] < 0) { snprintf(err, cap, "frame 0: feat_first %d is negative", I.feat_first[0]); return false; }
        for (int f = 0; f < I.n_frames; ++f) {
            if (I.feat_first[f + 1] < I.feat_first[f]) { snprintf(err, cap, "frame %d: feat_first descends (%d after %d)", f, I.feat_first[f + 1], I.feat_first[f]); return false; }
            const int n = I.feat_first[f + 1] - I.feat_first[f];
            if (n > GFW_FLOW_FEATURES_MAX) { snprintf(err, cap, "frame %d: %d features, at most %d", f, n, GFW_FLOW_FEATURES_MAX); return false; }
        }
        if (I.feat_first[I.n_frames] > I.feat_first[0] && !I.features) { snprintf(err, cap, "bad flow arguments (point mode 0 without features: %d features, null array)", I.feat_first[I.n_frames] - I.feat_first[0]); return false; }
    } else {
        const GfwFlowGrid G = gfw_flow_grid(I.width, I.height);
        if (G.nodes > GFW_FLOW_FEATURES_MAX) { snprintf(err, cap, "the grid of a %d x %d frame has %d nodes, at most %d", I.width, I.height, G.nodes, GFW_FLOW_FEATURES_MAX); return false; }
    }
    for (int p = 0; p < I.n_pairs; ++p) {
        const int a = I.pair_frames[p * 2], b = I.pair_frames[p * 2 + 1];
        if (a < 0 || a >= I.n_frames || b < 0 || b >= I.n_frames) { snprintf(err, cap, "pair %d: frames (%d, %d) outside the call's %d frames", p, a, b, I.n_frames); return false; }
        if (a == b) { snprintf(err, cap, "pair %d: frame %d paired with itself", p, a); return false; }
    }
    const GfwFlowPlan P = gfw_flow_plan(I);                  // (every index it reads has just been checked)
    if (P.total > GFW_FLOW_STAGED_MAX) {
        snprintf(err, cap, "the call stages %zu bytes (%d frames of stride %d x %d rows, %d features): at most 2 GiB", P.total, I.frames_on_device ? 0 : I.n_frames, I.stride, I.height, P.n_features); return false; }
    return true;
}

// Fills the block at (h, d) and the argument block's inputs, kept counts, levels (level l's work space at `pyramid` + level_at[l]) and counts
inline void gfw_flow_fill(const GfwFlowPlan &P, const GfwFlowInputs &I, char *h, char *d, const uint8_t *pyramid, GfwFlowArgs &A) {
    memcpy(h + P.o_pairs, I.pair_frames, sizeof(int32_t) * 2 * (size_t)I.n_pairs);
    int32_t *raw = (int32_t *)(h + P.o_raw);
    raw[0] = 0;
    for (int p = 0; p < I.n_pairs; ++p) {
        const int a = I.pair_frames[p * 2];
        raw[p + 1] = raw[p] + (I.mode == GFW_FLOW_MODE_GRID ? P.grid.nodes : I.feat_first[a + 1] - I.feat_first[a]);
    }
    memset(h + P.o_kept, 0, sizeof(int32_t) * (size_t)I.n_pairs);
    A.kept = (int32_t *)(d + P.o_kept);
    A.feat_first = nullptr; A.features = nullptr;
    if (I.mode == GFW_FLOW_MODE_FEATURES) {
        int32_t *ff = (int32_t *)(h + P.o_ffirst);
        for (int f = 0; f <= I.n_frames; ++f) ff[f] = I.feat_first[f] - I.feat_first[0];
        if (P.n_features) memcpy(h + P.o_feat, I.features + (size_t)I.feat_first[0] * 2, sizeof(float) * 2 * (size_t)P.n_features);
        A.feat_first = (const int32_t *)(d + P.o_ffirst); A.features = (const float *)(d + P.o_feat);
    }
    const uint8_t *frames = (const uint8_t *)I.frames;
    if (!I.frames_on_device) {
        if (I.n_frames) memcpy(h + P.o_frames, I.frames, P.frame_bytes * (size_t)I.n_frames);
        frames = (const uint8_t *)(d + P.o_frames);
    }
    A.lv[0] = GfwFlowLevel{frames, (int64_t)P.frame_bytes, I.width, I.height, I.stride, 0};
    for (int l = 1; l < GFW_FLOW_LEVELS; ++l) {
        if (l <= P.top) A.lv[l] = GfwFlowLevel{pyramid + P.level_at[l], (int64_t)P.lw[l] * P.lh[l], P.lw[l], P.lh[l], P.lw[l], 0};
        else A.lv[l] = GfwFlowLevel{nullptr, 0, 0, 0, 0, 0};
    }
    A.pair_frames = (const int32_t *)(d + P.o_pairs); A.raw_first = (const int32_t *)(d + P.o_raw);
    A.top = P.top; A.n_frames = I.n_frames; A.n_pairs = I.n_pairs; A.mode = I.mode; A.max_features = P.max_features;
    A.grid_step = P.grid.step; A.grid_half = P.grid.half; A.grid_rows = P.grid.rows; A.grid_nodes = P.grid.nodes;
}
