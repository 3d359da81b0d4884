// gfw_pose_essential_host.h — host only: what gfw_pose_essential checks and stages for the kernels of gfw_pose_essential.hip (its draws, gfw_pose_draws_k, are
// gfw_pose_host.h's, beside the generator they share).  Included behind gfw_pose_essential.h (GfwPoseEssArgs) by gfw_api.hip and by whatever else stages a call for
// those kernels; no kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include "gfw_pairs_host.h"

// The caller's arrays of one call (include/gfwarp.h: gfw_pose_essential)
struct GfwPoseEssInputs {
    const int32_t *pair_first; const float *points_a, *points_b; int n_pairs;
    GfwPairSet pairs() const { return GfwPairSet{nullptr, pair_first, points_a, points_b, n_pairs}; }
    const int32_t *octets;
    int num_iters;
};

// -> true, or false with the reason (the pair named) in `err`
inline bool gfw_pose_ess_check(const GfwPoseEssInputs &I, char *err, size_t cap) {
    int total, max_pair;
    if (I.n_pairs < 0 || I.num_iters < 0) { snprintf(err, cap, "bad pose arguments (negative count: %d pairs, %d rounds)", I.n_pairs, I.num_iters); return false; }
    if (!gfw_pairs_check(I.pairs(), {"pose", GFW_PE_PAIRS_MAX, GFW_PE_PAIR_MAX, false, false}, total, max_pair, err, cap)) return false;
    if (I.num_iters > GFW_PE_ROUNDS_MAX) { snprintf(err, cap, "%d rounds: at most %d", I.num_iters, GFW_PE_ROUNDS_MAX); return false; }
    if (I.n_pairs == 0) return true;
    if (I.num_iters && !I.octets) { snprintf(err, cap, "bad pose arguments (rounds without octets)"); return false; }
    for (int p = 0; p < I.n_pairs; ++p) {
        const int n = I.pair_first[p + 1] - I.pair_first[p];
        if (n < GFW_PE_MIN_POINTS) continue;                                          // its octets are ignored
        const int32_t *o = I.octets + (size_t)p * I.num_iters * 8;
        for (int it = 0; it < I.num_iters; ++it, o += 8) {
            for (int k = 0; k < 8; ++k) {
                if (o[k] < 0 || o[k] >= n) { snprintf(err, cap, "pair %d: round %d draws %d outside its %d points", p, it, o[k], n); return false; }
                for (int j = 0; j < k; ++j)
                    if (o[j] == o[k]) { snprintf(err, cap, "pair %d: round %d draws a point twice (%d)", p, it, o[k]); return false; }
            }
        }
    }
    return true;
}

// The staged block: [n_pairs + 1] first points, the points of the first frames then of the second, the octets.
struct GfwPoseEssLayout { size_t o_first, o_pts, o_octets, total; };
inline GfwPoseEssLayout gfw_pose_ess_layout(const GfwPoseEssInputs &I) {
    BlockLayout L;
    GfwPoseEssLayout S;
    gfw_pairs_add(L, I.n_pairs, (size_t)gfw_pairs_total(I.pairs(), false), S.o_first, S.o_pts);
    S.o_octets = L.add(sizeof(int32_t) * 8 * (size_t)I.n_pairs * (size_t)I.num_iters);
    S.total = L.total;
    return S;
}
// Fills the block at (h, d) and the argument block's input pointers and counts
inline void gfw_pose_ess_fill(const GfwPoseEssLayout &S, const GfwPoseEssInputs &I, char *h, const char *d, GfwPoseEssArgs &A) {
    A.total = gfw_pairs_fill(S.o_first, S.o_pts, I.pairs(), false, h, d, A.pair_first, A.points);
    if (I.n_pairs && I.num_iters) memcpy(h + S.o_octets, I.octets, sizeof(int32_t) * 8 * (size_t)I.n_pairs * (size_t)I.num_iters);
    A.octets = (const int32_t *)(d + S.o_octets); A.n_pairs = I.n_pairs; A.num_iters = I.num_iters;
}
// The call's constants
inline void gfw_pose_ess_constants(int video_w, int video_h, int flow_w, int flow_h, double inlier_threshold, int min_front, GfwPoseEssArgs &A) {
    A.vw = (float)video_w; A.vh = (float)video_h; A.fw = (float)flow_w; A.fh = (float)flow_h;
    A.threshold = inlier_threshold; A.min_front = min_front;
}
