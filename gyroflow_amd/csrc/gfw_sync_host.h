// gfw_sync_host.h — host only: what gfw_sync_visual_costs / gfw_sync_visual_search check and stage for the kernels of gfw_sync.hip, and the gyro low-pass of the gyro-match
// search (gfw_lowpass_gyro).  Included behind gfw_sync.h (GfwSyncArgs) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit
// sees it and it calls nothing of HIP.
#pragma once
#include <math.h>
#include <cmath>
#include "gfw_pairs_host.h"

// The staged block: [n_pairs][2] timestamps, [n_pairs + 1] first points, the points of the first frames then of the second, [n][2] candidates.
struct GfwSyncLayout { size_t o_ts, o_first, o_pts, o_cand, total; };
inline GfwSyncLayout gfw_sync_layout(int n_pairs, int total_points, size_t n_candidates) {
    BlockLayout L;
    GfwSyncLayout S;
    S.o_ts = L.add(sizeof(int64_t) * 2 * (size_t)n_pairs);
    gfw_pairs_add(L, n_pairs, (size_t)total_points, S.o_first, S.o_pts);
    S.o_cand = L.add(sizeof(double) * 2 * n_candidates);
    S.total = L.total;
    return S;
}
// The first stage's steps: `search_size as usize` (visual_features.rs:113) / `(1000.0 / fps) as isize`, `-steps..steps` (:89-91): saturating casts, NaN -> 0.
// A double, for the entry point to refuse what is too many; the candidates are steps (mode 0) or 2 * steps (mode 1)
inline double gfw_sync_coarse_steps(int mode, double search_size_ms, double scaled_fps) {
    const double v = mode == 0 ? search_size_ms : 1000.0 / scaled_fps;
    return !(v == v) || v <= 0.0 ? 0.0 : trunc(v);
}
// What gfw_sync_visual_costs (`mode` < 0: `out` is its costs) / gfw_sync_visual_search (`mode` 0 / 1: `out` is its result) refuse without looking at the context;
// `flags` are the kernel parameters'.  -> true with the pair set's counts (gfw_pairs_check) and the coarse candidates' count, or false with the reason in `err`
inline bool gfw_sync_check(const gfw_sync_search *search, int flags, const GfwPairSet &P, const double *candidates, int n_candidates, int mode, double search_size_ms,
                           double scaled_fps, const void *out, int &total, int &max_pair, int &n_coarse, char *err, size_t cap) {
    if (!search || P.n_pairs < 0 || n_candidates < 0) { snprintf(err, cap, "bad sync arguments (null context / params / search, or a negative count)"); return false; }
    if (search->reserved[0] || search->reserved[1]) { snprintf(err, cap, "bad sync search: reserved slots must be 0"); return false; }
    if (search->width < 1 || search->height < 1 || search->horizontal_readout < 0 || search->horizontal_readout > 1 || search->use_sync_offsets < 0 || search->use_sync_offsets > 1) {
        snprintf(err, cap, "bad sync search: %d x %d, horizontal_readout %d, use_sync_offsets %d", search->width, search->height, search->horizontal_readout, search->use_sync_offsets);
        return false; }
    if ((unsigned long long)search->width * (unsigned long long)search->width + (unsigned long long)search->height * (unsigned long long)search->height >= (1ull << 32)) {
        snprintf(err, cap, "bad sync search: %d x %d — width^2 + height^2 must stay below 2^32 (a squared distance is folded as 32 bits)", search->width, search->height);
        return false; }
    if (!gfw_pairs_lens_flags(flags, "the sync search", err, cap) || !gfw_pairs_check(P, {"sync", GFW_SYNC_PAIRS_MAX, GFW_SYNC_PAIR_MAX, true, false}, total, max_pair, err, cap)) return false;
    n_coarse = n_candidates;
    if (mode < 0) {
        if (n_candidates && (!candidates || !out)) { snprintf(err, cap, "bad sync arguments (candidates without their array / costs)"); return false; }
    } else {
        if (mode > 1 || !out) { snprintf(err, cap, "bad sync arguments (mode %d, or a null result)", mode); return false; }
        const double steps = gfw_sync_coarse_steps(mode, search_size_ms, scaled_fps);
        if (steps > 1000000.0) { snprintf(err, cap, "a search of %g candidates (search_size_ms %g, scaled_fps %g)", steps * (mode ? 2.0 : 1.0), search_size_ms, scaled_fps); return false; }
        n_coarse = (int)steps * (mode ? 2 : 1);
    }
    return true;
}
// Fills the block at (h, d) and the argument block's input pointers.  `candidates` nullptr: the `n_candidates` coarse ones of `mode` are made here (:113-115, :89-91)
inline void gfw_sync_fill(const GfwSyncLayout &S, const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                          const double *candidates, int n_candidates, int mode, double initial_offset_ms, double search_size_ms, double frame_readout_time_ms,
                          char *h, const char *d, GfwSyncArgs &A) {
    const GfwPairSet P = {pair_ts_us, pair_first, points_a, points_b, n_pairs};
    if (P.n_pairs) memcpy(h + S.o_ts, P.pair_ts_us, sizeof(int64_t) * 2 * (size_t)P.n_pairs);
    A.total = gfw_pairs_fill(S.o_first, S.o_pts, P, false, h, d, A.pair_first, A.points);
    double *hc = (double *)(h + S.o_cand);
    if (candidates) memcpy(hc, candidates, sizeof(double) * 2 * (size_t)n_candidates);
    else for (int i = 0; i < n_candidates; ++i) {
        if (mode == 0) { hc[i * 2] = initial_offset_ms + (-(search_size_ms / 2.0) + (double)i); hc[i * 2 + 1] = frame_readout_time_ms; }
        else { hc[i * 2] = 0.0; hc[i * 2 + 1] = (double)(i - n_candidates / 2); }
    }
    A.pair_ts = (const int64_t *)(d + S.o_ts); A.candidates = (const double *)(d + S.o_cand);
    A.n_pairs = P.n_pairs;
}

// Lowpass::filter_gyro_forward_backward (filtering.rs:46-74) of a gyro triple series, in place: biquad's second-order Butterworth low-pass (Q = FRAC_1_SQRT_2) in
// transposed direct form II, forward then backward, one filter per axis and direction; entries without a gyro do not advance the state.  -> false: not applied
inline bool gfw_lowpass_gyro_host(double freq, double sample_rate, double *xyz, const uint8_t *has, int n) {
    // Coefficients::from_params fails for 2 f0 > fs (and the reference ignores the failure: essential_matrix.rs:47-48)
    if (!std::isfinite(freq) || !std::isfinite(sample_rate) || !(freq > 0.0) || !(sample_rate > 0.0) || 2.0 * freq > sample_rate) return false;
    const double omega = 2.0 * 3.14159265358979323846 * freq / sample_rate;
    const double omega_s = sin(omega), omega_c = cos(omega);
    const double alpha = omega_s / (2.0 * 0.70710678118654752440);
    const double b0 = (1.0 - omega_c) * 0.5, b1 = 1.0 - omega_c, b2 = (1.0 - omega_c) * 0.5;
    const double a0 = 1.0 + alpha, a1 = -2.0 * omega_c, a2 = 1.0 - alpha;
    const double cb0 = b0 / a0, cb1 = b1 / a0, cb2 = b2 / a0, ca1 = a1 / a0, ca2 = a2 / a0;
    for (int pass = 0; pass < 2; ++pass) {
        double s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < n; ++k) {
            const int i = pass ? n - 1 - k : k;
            if (has && !has[i]) continue;
            for (int a = 0; a < 3; ++a) {
                const double x = xyz[(size_t)i * 3 + a];
                const double out = s1[a] + cb0 * x;
                s1[a] = s2[a] + cb1 * x - ca1 * out;
                s2[a] = cb2 * x - ca2 * out;
                xyz[(size_t)i * 3 + a] = out;
            }
        }
    }
    return true;
}
