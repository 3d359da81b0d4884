// gfw_dis_host.h — host only: what gfw_flow_dis checks, sizes and stages for the kernels of gfw_dis.hip.  Included behind gfw_dis.h (GfwDisArgs), gfw_flow.h and gfw_flow_host.h
// (GfwFlowArgs and the grid of opencv_dis.rs:62-72, which is gfw_flow_pyrlk's point mode 1 unchanged) by gfw_api.hip and by whatever else stages a call for those kernels; no
// kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "gfw_layout.h"

// The caller's arguments of one call (include/gfwarp.h: gfw_flow_dis)
struct GfwDisInputs {
    int width, height, stride, finest, variational_iters, reserved;
    const void *frames; int frames_on_device, n_frames;
    const int32_t *pair_frames; int n_pairs;
};

// min(int(log2(max(w, h) / 32) + 0.5), int(log2(min(w, h) / 8))) in integers, for sides >= 1: the first term is the largest k with 32 * 2^(k - 0.5) <= max, that is
// max^2 >= 512 * 4^k (never an equality: 512 * 4^k is no square), or <= 0 where there is none — the C cast truncates -0.5 and up to 0, and what lies below is under
// every finest scale anyway —; the second is the largest k with 8 * 2^k <= min, or negative where min < 8.
inline int gfw_dis_coarsest(int width, int height) {
    const int64_t big = width > height ? width : height, small = width > height ? height : width;
    int a = 0, b = -1;
    while (big * big >= ((int64_t)512 << (2 * (a + 1)))) ++a;
    while (small >= ((int64_t)8 << (b + 1))) ++b;
    return a < b ? a : b;
}
// The sides of levels 0 .. coarsest (level l + 1: w_l / 2, h_l / 2) -> coarsest (negative: no level at all)
inline int gfw_dis_levels(int width, int height, int *lw, int *lh) {
    const int coarsest = gfw_dis_coarsest(width, height);
    for (int l = 0; l < GFW_DIS_LEVELS; ++l) { lw[l] = 0; lh[l] = 0; }
    lw[0] = width; lh[0] = height;
    for (int l = 1; l <= coarsest && l < GFW_DIS_LEVELS; ++l) { lw[l] = lw[l - 1] / 2; lh[l] = lh[l - 1] / 2; }
    return coarsest;
}
inline int gfw_dis_patches(int w, int h) { return ((w - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1) * ((h - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1); }

// What a call with pairs needs: the levels, the grid, the device work space (levels 1 .. coarsest of every frame, the dense fields of levels finest .. coarsest —
// the entry point writes the finest one straight to the caller's `flow` where that is asked for —, the patch values of three passes at the level with the most patches: the finest) and
// the staged block: [n_pairs][2] frames, then the frames where they are host memory.
struct GfwDisPlan {
    int coarsest, lw[GFW_DIS_LEVELS], lh[GFW_DIS_LEVELS];
    GfwFlowGrid grid;
    int64_t points_max;                                                      // room the caller's points_a / points_b have: every node of the grid per pair
    size_t frame_bytes, level_at[GFW_DIS_LEVELS], dense_at[GFW_DIS_LEVELS], dense_bytes[GFW_DIS_LEVELS], patch_at[3], work_bytes;
    size_t o_pairs, o_frames, total;
};
inline GfwDisPlan gfw_dis_plan(const GfwDisInputs &I) {
    GfwDisPlan P;
    memset(&P, 0, sizeof(P));
    P.coarsest = gfw_dis_levels(I.width, I.height, P.lw, P.lh);
    P.grid = gfw_flow_grid(I.width, I.height);
    P.points_max = (int64_t)P.grid.nodes * I.n_pairs;
    P.frame_bytes = (size_t)I.stride * (size_t)I.height;
    BlockLayout W;
    for (int l = 1; l <= P.coarsest; ++l) P.level_at[l] = W.add((size_t)I.n_frames * (size_t)P.lw[l] * (size_t)P.lh[l]);
    for (int l = I.finest; l <= P.coarsest; ++l) {
        P.dense_bytes[l] = sizeof(float) * 2 * (size_t)I.n_pairs * (size_t)P.lw[l] * (size_t)P.lh[l];
        P.dense_at[l] = W.add(P.dense_bytes[l]);
    }
    for (int k = 0; k < 3; ++k) P.patch_at[k] = W.add(sizeof(float) * 2 * (size_t)I.n_pairs * (size_t)gfw_dis_patches(P.lw[I.finest], P.lh[I.finest]));
    P.work_bytes = W.total;
    BlockLayout L;
    P.o_pairs = L.add(sizeof(int32_t) * 2 * (size_t)I.n_pairs);
    P.o_frames = L.add(I.frames_on_device ? 0 : P.frame_bytes * (size_t)I.n_frames);
    P.total = L.total;
    return P;
}
// -> true, or false with the reason (the pair or frame named) in `err`
inline bool gfw_dis_check(const GfwDisInputs &I, char *err, size_t cap) {
    if (I.reserved) { snprintf(err, cap, "bad DIS flow configuration: the reserved slot must be 0"); return false; }
    if (I.variational_iters) { snprintf(err, cap, "bad DIS flow configuration: variational_iters %d (it must be 0 here: variational refinement is gfw_flow_dis_refined's, counted in its gfw_flow_varref_cfg)", I.variational_iters); return false; }
    if (I.finest != 1 && I.finest != 2) { snprintf(err, cap, "bad DIS flow configuration: finest_scale %d (1 or 2)", I.finest); return false; }
    if (I.n_frames < 0 || I.n_pairs < 0) { snprintf(err, cap, "bad DIS flow arguments (negative count: %d frames, %d pairs)", I.n_frames, I.n_pairs); return false; }
    if (I.width < 1 || I.width > GFW_DIS_SIDE_MAX || I.height < 1 || I.height > GFW_DIS_SIDE_MAX) {
        snprintf(err, cap, "bad DIS flow configuration: frames of %d x %d, both sides must be between 1 and %d", I.width, I.height, GFW_DIS_SIDE_MAX); return false; }
    const int coarsest = gfw_dis_coarsest(I.width, I.height);
    if (coarsest < I.finest) {
        snprintf(err, cap, "bad DIS flow configuration: frames of %d x %d have the coarsest scale %d, under the finest scale %d", I.width, I.height, coarsest, I.finest); return false; }
    if (I.stride < I.width) { snprintf(err, cap, "bad DIS flow configuration: stride %d under the width %d", I.stride, I.width); return false; }
    if (I.n_frames > GFW_DIS_FRAMES_MAX) { snprintf(err, cap, "%d frames: at most %d in a call", I.n_frames, GFW_DIS_FRAMES_MAX); return false; }
    if (I.n_pairs > GFW_DIS_PAIRS_MAX) { snprintf(err, cap, "%d pairs: at most %d in a call", I.n_pairs, GFW_DIS_PAIRS_MAX); return false; }
    if (I.n_pairs == 0) return true;
    if (!I.pair_frames) { snprintf(err, cap, "bad DIS flow arguments (pairs without pair_frames)"); return false; }
    if (I.n_frames && !I.frames) { snprintf(err, cap, "bad DIS flow arguments (%d frames without their planes)", I.n_frames); return false; }
    const GfwFlowGrid G = gfw_flow_grid(I.width, I.height);                  // (coarsest >= 1: both sides are >= 16, the grid's step is >= 1)
    if (G.nodes > GFW_DIS_NODES_MAX) { snprintf(err, cap, "the grid of a %d x %d frame has %d nodes, at most %d", I.width, I.height, G.nodes, GFW_DIS_NODES_MAX); return false; }
    for (int p = 0; p < I.n_pairs; ++p) {
        const int a = I.pair_frames[p * 2], b = I.pair_frames[p * 2 + 1];
        if (a < 0 || a >= I.n_frames || b < 0 || b >= I.n_frames) { snprintf(err, cap, "pair %d: frames (%d, %d) outside the call's %d frames", p, a, b, I.n_frames); return false; }
        if (a == b) { snprintf(err, cap, "pair %d: frame %d paired with itself", p, a); return false; }
    }
    const GfwDisPlan P = gfw_dis_plan(I);
    if (P.total > GFW_DIS_STAGED_MAX) {
        snprintf(err, cap, "the call stages %zu bytes (%d frames of stride %d x %d rows): at most 2 GiB", P.total, I.frames_on_device ? 0 : I.n_frames, I.stride, I.height); return false; }
    if (P.work_bytes > GFW_DIS_WORK_MAX) {
        snprintf(err, cap, "the call needs %zu bytes of device work space (%d pairs, %d frames of %d x %d at the finest scale %d): at most 16 GiB", P.work_bytes, I.n_pairs, I.n_frames, I.width, I.height, I.finest); return false; }
    return true;
}

// Fills the block at (h, d) and the argument blocks' inputs: the levels (level l's work space at `work` + level_at[l]), the dense fields and patch values in the work
// space, the counts; G is what gfw_launch_flow_grid takes (the caller sets both blocks' grid_points / grid_counts and A's outputs)
inline void gfw_dis_fill(const GfwDisPlan &P, const GfwDisInputs &I, char *h, char *d, char *work, GfwDisArgs &A, GfwFlowArgs &G) {
    memcpy(h + P.o_pairs, I.pair_frames, sizeof(int32_t) * 2 * (size_t)I.n_pairs);
    const uint8_t *frames = (const uint8_t *)I.frames;
    if (!I.frames_on_device) {
        if (I.n_frames) memcpy(h + P.o_frames, I.frames, P.frame_bytes * (size_t)I.n_frames);
        frames = (const uint8_t *)(d + P.o_frames);
    }
    A.lv[0] = GfwDisLevel{frames, (int64_t)P.frame_bytes, I.width, I.height, I.stride, 0};
    for (int l = 1; l < GFW_DIS_LEVELS; ++l) {
        if (l <= P.coarsest) A.lv[l] = GfwDisLevel{(const uint8_t *)work + P.level_at[l], (int64_t)P.lw[l] * P.lh[l], P.lw[l], P.lh[l], P.lw[l], 0};
        else A.lv[l] = GfwDisLevel{nullptr, 0, 0, 0, 0, 0};
    }
    for (int l = 0; l < GFW_DIS_LEVELS; ++l) A.dense[l] = l >= I.finest && l <= P.coarsest ? (float *)(work + P.dense_at[l]) : nullptr;
    for (int k = 0; k < 3; ++k) A.patch[k] = (float *)(work + P.patch_at[k]);
    A.pair_frames = (const int32_t *)(d + P.o_pairs);
    A.coarsest = P.coarsest; A.finest = I.finest; A.n_frames = I.n_frames; A.n_pairs = I.n_pairs; A.grid_nodes = P.grid.nodes;
    G.lv[0] = GfwFlowLevel{frames, (int64_t)P.frame_bytes, I.width, I.height, I.stride, 0};
    G.n_frames = I.n_frames; G.n_pairs = I.n_pairs; G.mode = GFW_FLOW_MODE_GRID;
    G.grid_step = P.grid.step; G.grid_half = P.grid.half; G.grid_rows = P.grid.rows; G.grid_nodes = P.grid.nodes;
}
