// gfw_sync_host.h — host only: what gfw_sync_visual_costs / gfw_sync_visual_search stage for the kernels of gfw_sync.hip, and the gyro low-pass of the gyro-match
// search (gfw_lowpass_gyro).  Included behind gfw_sync.h (GfwSyncArgs) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit
// sees it, it calls nothing of HIP and reports no errors (the entry points validate).
#pragma once
#include <math.h>
#include <string.h>
#include <cmath>
#include "gfw_layout.h"

// The staged block: [n_pairs][2] timestamps, [n_pairs + 1] first points, the points of the first frames then of the second, [n][2] candidates.
struct GfwSyncLayout { size_t o_ts, o_first, o_pts, o_cand, total; };
inline GfwSyncLayout gfw_sync_layout(int n_pairs, int total_points, size_t n_candidates) {
    BlockLayout L;
    GfwSyncLayout S;
    S.o_ts = L.add(sizeof(int64_t) * 2 * (size_t)n_pairs);
    S.o_first = L.add(sizeof(int32_t) * ((size_t)n_pairs + 1));
    S.o_pts = L.add(sizeof(float) * 2 * (size_t)total_points * 2);
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
// Fills the block at (h, d) and the argument block's input pointers.  `candidates` nullptr: the `n_candidates` coarse ones of `mode` are made here (:113-115, :89-91)
inline void gfw_sync_fill(const GfwSyncLayout &S, const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                          const double *candidates, int n_candidates, int mode, double initial_offset_ms, double search_size_ms, double frame_readout_time_ms,
                          char *h, const char *d, GfwSyncArgs &A) {
    const int total = n_pairs ? pair_first[n_pairs] : 0;
    const size_t pb = sizeof(float) * 2 * (size_t)total;
    if (n_pairs) { memcpy(h + S.o_ts, pair_ts_us, sizeof(int64_t) * 2 * (size_t)n_pairs); memcpy(h + S.o_first, pair_first, sizeof(int32_t) * ((size_t)n_pairs + 1)); }
    else *(int32_t *)(h + S.o_first) = 0;
    if (total) { memcpy(h + S.o_pts, points_a, pb); memcpy(h + S.o_pts + pb, points_b, pb); }
    double *hc = (double *)(h + S.o_cand);
    if (candidates) memcpy(hc, candidates, sizeof(double) * 2 * (size_t)n_candidates);
    else for (int i = 0; i < n_candidates; ++i) {
        if (mode == 0) { hc[i * 2] = initial_offset_ms + (-(search_size_ms / 2.0) + (double)i); hc[i * 2 + 1] = frame_readout_time_ms; }
        else { hc[i * 2] = 0.0; hc[i * 2 + 1] = (double)(i - n_candidates / 2); }
    }
    A.pair_ts = (const int64_t *)(d + S.o_ts); A.pair_first = (const int32_t *)(d + S.o_first); A.points = (const float *)(d + S.o_pts);
    A.candidates = (const double *)(d + S.o_cand);
    A.n_pairs = n_pairs; A.total = total;
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
