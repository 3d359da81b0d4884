// gfw_pose_host.h — host only: what gfw_pose_almeida checks and stages for the kernels of gfw_pose.hip, and the draws of gfw_pose_draws.  Included behind gfw_pose.h
// (GfwPoseArgs, gfw_pose_math.h) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include "gfw_pairs_host.h"

// The caller's arrays of one call (include/gfwarp.h: gfw_pose_almeida)
struct GfwPoseInputs {
    const int32_t *pair_first; const float *points_a, *points_b; int n_pairs;
    GfwPairSet pairs() const { return GfwPairSet{nullptr, pair_first, points_a, points_b, n_pairs}; }
    const int32_t *triples, *sample_first, *samples;
    int num_iters, num_samples;
};
inline int gfw_pose_list_len(int n, int num_samples) { return n < num_samples ? n : num_samples; }

// -> true, or false with the reason (the pair named) in `err`
inline bool gfw_pose_check(const GfwPoseInputs &I, char *err, size_t cap) {
    int total, max_pair;
    if (I.n_pairs < 0 || I.num_iters < 0 || I.num_samples < 0) { snprintf(err, cap, "bad pose arguments (negative count: %d pairs, %d rounds, %d samples)", I.n_pairs, I.num_iters, I.num_samples); return false; }
    if (!gfw_pairs_check(I.pairs(), {"pose", GFW_POSE_PAIRS_MAX, GFW_POSE_PAIR_MAX, false, false}, total, max_pair, err, cap)) return false;
    if (I.num_iters > GFW_POSE_ROUNDS_MAX) { snprintf(err, cap, "%d rounds: at most %d", I.num_iters, GFW_POSE_ROUNDS_MAX); return false; }
    if (I.n_pairs == 0) return true;
    if (!I.samples && max_pair > I.num_samples) for (int p = 0; p < I.n_pairs; ++p)
        if (I.pair_first[p + 1] - I.pair_first[p] > I.num_samples) { snprintf(err, cap, "pair %d: %d points but num_samples %d, and no sample lists", p, I.pair_first[p + 1] - I.pair_first[p], I.num_samples); return false; }
    if (I.num_iters && !I.triples) { snprintf(err, cap, "bad pose arguments (rounds without triples)"); return false; }
    if (I.samples && !I.sample_first) { snprintf(err, cap, "bad pose arguments (samples without sample_first)"); return false; }
    if (I.samples && I.sample_first[0] < 0) { snprintf(err, cap, "pair 0: sample_first %d is negative", I.sample_first[0]); return false; }
    for (int p = 0; p < I.n_pairs; ++p) {
        const int n = I.pair_first[p + 1] - I.pair_first[p];
        if (n >= 3) {
            const int32_t *t = I.triples + (size_t)p * I.num_iters * 3;
            for (int it = 0; it < I.num_iters; ++it, t += 3) {
                if (t[0] < 0 || t[0] >= n || t[1] < 0 || t[1] >= n || t[2] < 0 || t[2] >= n) {
                    snprintf(err, cap, "pair %d: round %d draws (%d, %d, %d) outside its %d points", p, it, t[0], t[1], t[2], n); return false; }
                if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) { snprintf(err, cap, "pair %d: round %d draws a point twice (%d, %d, %d)", p, it, t[0], t[1], t[2]); return false; }
            }
        }
        if (I.samples) {
            const long long want = (long long)I.num_iters * gfw_pose_list_len(n, I.num_samples), got = (long long)I.sample_first[p + 1] - I.sample_first[p];
            if (got != want) { snprintf(err, cap, "pair %d: %lld sample entries (sample_first %d .. %d), %lld wanted", p, got, I.sample_first[p], I.sample_first[p + 1], want); return false; }
            const int32_t *s = I.samples + I.sample_first[p];
            for (long long k = 0; k < want; ++k)
                if (s[k] < 0 || s[k] >= n) { snprintf(err, cap, "pair %d: sample %d of round %lld outside its %d points", p, s[k], k / gfw_pose_list_len(n, I.num_samples), n); return false; }
        }
    }
    return true;
}

// The staged block: [n_pairs + 1] first points, the points of the first frames then of the second, the triples, and with sample lists [n_pairs + 1] firsts (from 0) and the lists.
struct GfwPoseLayout { size_t o_first, o_pts, o_triples, o_sfirst, o_samples, total; };
inline GfwPoseLayout gfw_pose_layout(const GfwPoseInputs &I) {
    BlockLayout L;
    GfwPoseLayout S;
    gfw_pairs_add(L, I.n_pairs, (size_t)gfw_pairs_total(I.pairs(), false), S.o_first, S.o_pts);
    S.o_triples = L.add(sizeof(int32_t) * 3 * (size_t)I.n_pairs * (size_t)I.num_iters);
    S.o_sfirst = L.add(I.samples ? sizeof(int32_t) * ((size_t)I.n_pairs + 1) : 0);
    S.o_samples = L.add(I.samples && I.n_pairs ? sizeof(int32_t) * (size_t)(I.sample_first[I.n_pairs] - I.sample_first[0]) : 0);
    S.total = L.total;
    return S;
}
// Fills the block at (h, d) and the argument block's input pointers and counts
inline void gfw_pose_fill(const GfwPoseLayout &S, const GfwPoseInputs &I, char *h, const char *d, GfwPoseArgs &A) {
    A.total = gfw_pairs_fill(S.o_first, S.o_pts, I.pairs(), false, h, d, A.pair_first, A.points);
    if (I.n_pairs && I.num_iters) memcpy(h + S.o_triples, I.triples, sizeof(int32_t) * 3 * (size_t)I.n_pairs * (size_t)I.num_iters);
    A.sample_first = nullptr; A.samples = nullptr;
    if (I.samples && I.n_pairs) {
        int32_t *sf = (int32_t *)(h + S.o_sfirst);
        for (int p = 0; p <= I.n_pairs; ++p) sf[p] = I.sample_first[p] - I.sample_first[0];
        if (sf[I.n_pairs]) memcpy(h + S.o_samples, I.samples + I.sample_first[0], sizeof(int32_t) * (size_t)sf[I.n_pairs]);
        A.sample_first = (const int32_t *)(d + S.o_sfirst); A.samples = (const int32_t *)(d + S.o_samples);
    }
    A.triples = (const int32_t *)(d + S.o_triples); A.n_pairs = I.n_pairs; A.num_iters = I.num_iters; A.num_samples = I.num_samples;
}
// The call's constants: sizes, K in both precisions, the three derivative matrices, the inlier gate `inlier_angle.to_radians()` = angle * (PI / 180) in f32
inline void gfw_pose_constants(int video_w, int video_h, int flow_w, int flow_h, float inlier_angle_deg, const double *K, GfwPoseArgs &A) {
    for (int i = 0; i < 9; ++i) A.K[i] = K[i];
    gfw_pose_eps_matrices(K, A.eps_m);
    A.vw = (float)video_w; A.vh = (float)video_h; A.fw = (float)flow_w; A.fh = (float)flow_h;
    A.cx = (float)K[2]; A.cy = (float)K[5]; A.fx = (float)K[0]; A.fy = (float)K[4];
    A.target = inlier_angle_deg * (3.14159265358979323846f / 180.0f);
}

// gfw_pose_draws: a counter-based generator — word(seed, pair, round, k) = mix(mix(seed ^ (pair << 32 | round)) + k), mix the 64-bit finaliser of SplitMix64;
// a uniform index below r is the high word of (word >> 32) * r.  A round's triple is three distinct indices (the second and third drawn from what is left);
// its list is the first min(n, num_samples) entries of a Fisher-Yates shuffle of 0 .. n-1 (entry s swaps with one of s .. n-1).  One valid draw per seed, not rand's sequence.
inline uint64_t gfw_pose_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint32_t gfw_pose_below(uint64_t stream, uint64_t k, uint32_t r) { return (uint32_t)(((gfw_pose_mix(stream + k) >> 32) * (uint64_t)r) >> 32); }
inline bool gfw_pose_draws_host(uint64_t seed, const int32_t *pair_first, int n_pairs, int num_iters, int num_samples, int32_t *triples, const int32_t *sample_first, int32_t *samples) {
    if (n_pairs < 0 || num_iters < 0 || num_samples < 0 || (n_pairs && !pair_first) || (n_pairs && num_iters && !triples) || (samples && !sample_first)) return false;
    for (int p = 0; p < n_pairs; ++p) if (pair_first[p + 1] < pair_first[p] || pair_first[p + 1] - pair_first[p] > GFW_POSE_PAIR_MAX) return false;
    int32_t perm[GFW_POSE_PAIR_MAX];
    for (int p = 0; p < n_pairs; ++p) {
        const int n = pair_first[p + 1] - pair_first[p], m = gfw_pose_list_len(n, num_samples);
        if (samples && (long long)sample_first[p + 1] - sample_first[p] != (long long)num_iters * m) return false;
        for (int it = 0; it < num_iters; ++it) {
            const uint64_t stream = gfw_pose_mix(seed ^ (((uint64_t)(uint32_t)p << 32) | (uint32_t)it));
            int32_t *t = triples + ((size_t)p * num_iters + it) * 3;
            t[0] = t[1] = t[2] = 0;
            if (n >= 3) {
                int a = (int)gfw_pose_below(stream, 0, (uint32_t)n), b = (int)gfw_pose_below(stream, 1, (uint32_t)n - 1), c = (int)gfw_pose_below(stream, 2, (uint32_t)n - 2);
                if (b >= a) ++b;
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                if (c >= lo) ++c;
                if (c >= hi) ++c;
                t[0] = a; t[1] = b; t[2] = c;
            }
            if (samples) {
                int32_t *out = samples + sample_first[p] + (size_t)it * m;
                for (int i = 0; i < n; ++i) perm[i] = i;
                for (int s = 0; s < m; ++s) {
                    const int j = s + (int)gfw_pose_below(stream, 3 + (uint64_t)s, (uint32_t)(n - s));
                    const int32_t v = perm[j]; perm[j] = perm[s]; perm[s] = v;
                    out[s] = v;
                }
            }
        }
    }
    return true;
}

#define GFW_POSE_DRAWS_K_MAX 16     // distinct indices of a round
// gfw_pose_draws_k: the generator above for k distinct indices a round (the octets of gfw_pose_essential are k = 8).  Draw j is the
// r-th of the n - j indices not drawn yet, r = below(stream, j, n - j): r steps past every earlier draw in ascending order.  At k = 3 these are gfw_pose_draws'
// triples to the bit.  A pair under k points gets zeros.
inline bool gfw_pose_draws_k_host(uint64_t seed, const int32_t *pair_first, int n_pairs, int num_iters, int k, int32_t *tuples) {
    if (n_pairs < 0 || num_iters < 0 || k < 1 || k > GFW_POSE_DRAWS_K_MAX || (n_pairs && !pair_first) || (n_pairs && num_iters && !tuples)) return false;
    for (int p = 0; p < n_pairs; ++p) if (pair_first[p + 1] < pair_first[p] || pair_first[p + 1] - pair_first[p] > GFW_POSE_PAIR_MAX) return false;
    for (int p = 0; p < n_pairs; ++p) {
        const int n = pair_first[p + 1] - pair_first[p];
        for (int it = 0; it < num_iters; ++it) {
            const uint64_t stream = gfw_pose_mix(seed ^ (((uint64_t)(uint32_t)p << 32) | (uint32_t)it));
            int32_t *t = tuples + ((size_t)p * num_iters + it) * k;
            int32_t sorted[GFW_POSE_DRAWS_K_MAX];
            for (int j = 0; j < k; ++j) t[j] = 0;
            if (n < k) continue;
            for (int j = 0; j < k; ++j) {
                int r = (int)gfw_pose_below(stream, (uint64_t)j, (uint32_t)(n - j));
                int at = 0;
                for (; at < j && r >= sorted[at]; ++at) ++r;                          // past the earlier draws, ascending
                for (int m = j; m > at; --m) sorted[m] = sorted[m - 1];
                sorted[at] = r;
                t[j] = r;
            }
        }
    }
    return true;
}
