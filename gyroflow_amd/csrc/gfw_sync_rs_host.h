// gfw_sync_rs_host.h — host only: what gfw_sync_rs_costs / gfw_sync_rs_search check and stage for the kernels of gfw_sync_rs.hip.  Included behind gfw_sync_rs.h
// (GfwRsArgs) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include <math.h>
#include "gfw_pairs_host.h"

// The caller's arrays of one call (include/gfwarp.h: gfw_sync_rs_search)
struct GfwRsInputs {
    const int32_t *range_first; int n_ranges;
    const int64_t *pair_ts_us; const int32_t *pair_first; const float *points_a, *points_b; int n_pairs;
    GfwPairSet pairs() const { return GfwPairSet{pair_ts_us, pair_first, points_a, points_b, n_pairs}; }
    const int64_t *track_ts_us; const double *track_wxyz; int n_track;
    const int32_t *cand_first; const double *candidates; int n_candidates;      // gfw_sync_rs_costs only (cand_first null: a search)
};
// The solver's settings of one call (gfw_sync_rs_cfg's, and the search's two arguments)
struct GfwRsSettings { double step_s, initial_delay_s, radius_s, loss_scale; int rounds, refine, hypotheses, refits, sweeps; bool search; };

// candidates of round 0: 2 h + 1, h = floor(radius / step); -1 where they are more than GFW_RS_CANDIDATES_MAX
inline int gfw_rs_round0_count(double radius_s, double step_s) {
    const double h = floor(radius_s / step_s);
    return h * 2.0 + 1.0 > (double)GFW_RS_CANDIDATES_MAX ? -1 : 2 * (int)h + 1;
}

// -> true, or false with the reason (the range or pair named) in `err`
inline bool gfw_rs_check(const GfwRsInputs &I, const GfwRsSettings &S, char *err, size_t cap) {
    int points, max_pair;
    if (I.n_ranges < 0 || I.n_pairs < 0 || I.n_track < 0 || I.n_candidates < 0) {
        snprintf(err, cap, "bad rs-sync arguments (negative count: %d ranges, %d pairs, %d track samples, %d candidates)", I.n_ranges, I.n_pairs, I.n_track, I.n_candidates); return false; }
    if (I.n_ranges > GFW_RS_RANGES_MAX) { snprintf(err, cap, "%d ranges: at most %d in a call", I.n_ranges, GFW_RS_RANGES_MAX); return false; }
    if (I.n_pairs > GFW_RS_PAIRS_MAX) { snprintf(err, cap, "%d pairs: at most %d in a call", I.n_pairs, GFW_RS_PAIRS_MAX); return false; }      // here: also refused without ranges
    if (S.hypotheses < 0 || S.hypotheses > GFW_RS_HYPOTHESES_MAX || S.refits < 0 || S.refits > GFW_RS_REFITS_MAX || S.sweeps < 1 || S.sweeps > GFW_RS_SWEEPS_MAX || !(S.loss_scale > 0.0) || !isfinite(S.loss_scale)) {
        snprintf(err, cap, "bad rs-sync configuration: %d hypotheses (0 .. %d), %d refits (0 .. %d), %d Jacobi sweeps (1 .. %d), loss_scale %g", S.hypotheses, GFW_RS_HYPOTHESES_MAX, S.refits, GFW_RS_REFITS_MAX, S.sweeps, GFW_RS_SWEEPS_MAX, S.loss_scale);
        return false; }
    if (S.search) {
        if (!isfinite(S.step_s) || !(S.step_s > 0.0)) { snprintf(err, cap, "bad rs-sync search: step %g s is not a positive finite number", S.step_s); return false; }
        if (!isfinite(S.radius_s) || S.radius_s < 0.0) { snprintf(err, cap, "bad rs-sync search: radius %g s is negative or not finite", S.radius_s); return false; }
        if (!isfinite(S.initial_delay_s)) { snprintf(err, cap, "bad rs-sync search: initial delay %g s is not finite", S.initial_delay_s); return false; }
        if (S.rounds < 1 || S.rounds > GFW_RS_ROUNDS_MAX) { snprintf(err, cap, "bad rs-sync search: %d rounds, 1 .. %d", S.rounds, GFW_RS_ROUNDS_MAX); return false; }
        if (gfw_rs_round0_count(S.radius_s, S.step_s) < 0) { snprintf(err, cap, "bad rs-sync search: radius %g s at step %g s is more than %d candidates", S.radius_s, S.step_s, GFW_RS_CANDIDATES_MAX); return false; }
    }
    if (I.n_ranges == 0) return true;
    if (!I.range_first) { snprintf(err, cap, "bad rs-sync arguments (ranges without range_first)"); return false; }
    if (I.range_first[0] != 0) { snprintf(err, cap, "range 0: range_first %d is not 0", I.range_first[0]); return false; }
    for (int r = 0; r < I.n_ranges; ++r)
        if (I.range_first[r + 1] < I.range_first[r]) { snprintf(err, cap, "range %d: range_first descends (%d after %d)", r, I.range_first[r + 1], I.range_first[r]); return false; }
    if (I.range_first[I.n_ranges] != I.n_pairs) { snprintf(err, cap, "range %d: range_first ends at %d, the call has %d pairs", I.n_ranges - 1, I.range_first[I.n_ranges], I.n_pairs); return false; }
    if (!gfw_pairs_check(I.pairs(), {"rs-sync", GFW_RS_PAIRS_MAX, GFW_RS_PAIR_MAX, true, true}, points, max_pair, err, cap)) return false;      // the points count from pair_first[0]
    if (I.n_track < 2) { snprintf(err, cap, "a track of %d samples: at least 2", I.n_track); return false; }
    if (I.n_track > GFW_RS_TRACK_MAX) { snprintf(err, cap, "a track of %d samples: at most %d", I.n_track, GFW_RS_TRACK_MAX); return false; }
    if (!I.track_ts_us || !I.track_wxyz) { snprintf(err, cap, "bad rs-sync arguments (a null track array)"); return false; }
    for (int i = 1; i < I.n_track; ++i)
        if (I.track_ts_us[i] <= I.track_ts_us[i - 1]) { snprintf(err, cap, "track sample %d: timestamp %lld does not ascend (%lld before it)", i, (long long)I.track_ts_us[i], (long long)I.track_ts_us[i - 1]); return false; }
    if (!S.search) {
        if (!I.cand_first) { snprintf(err, cap, "bad rs-sync arguments (ranges without cand_first)"); return false; }
        if (I.cand_first[0] != 0) { snprintf(err, cap, "range 0: cand_first %d is not 0", I.cand_first[0]); return false; }
        for (int r = 0; r < I.n_ranges; ++r) {
            if (I.cand_first[r + 1] < I.cand_first[r]) { snprintf(err, cap, "range %d: cand_first descends (%d after %d)", r, I.cand_first[r + 1], I.cand_first[r]); return false; }
            if (I.cand_first[r + 1] - I.cand_first[r] > GFW_RS_CANDIDATES_MAX) { snprintf(err, cap, "range %d: %d candidates, at most %d", r, I.cand_first[r + 1] - I.cand_first[r], GFW_RS_CANDIDATES_MAX); return false; }
        }
        if (I.cand_first[I.n_ranges] != I.n_candidates) { snprintf(err, cap, "range %d: cand_first ends at %d, the call has %d candidates", I.n_ranges - 1, I.cand_first[I.n_ranges], I.n_candidates); return false; }
        if (I.n_candidates && !I.candidates) { snprintf(err, cap, "bad rs-sync arguments (%d candidates without their array)", I.n_candidates); return false; }
    }
    return true;
}

// The staged block: range firsts, the range of each pair, pair firsts (from 0), pair timestamps, the points of the first frames then of the second, the track as
// seconds and its quaternions; for caller-given candidates also their firsts, the candidates and each pair's first entry among the pair costs.
struct GfwRsLayout { size_t o_rfirst, o_prange, o_pfirst, o_pts_us, o_pts, o_tt, o_tq, o_cfirst, o_cand, o_pcfirst, total; size_t points, pair_costs; int max_cand, max_pair; };
inline GfwRsLayout gfw_rs_layout(const GfwRsInputs &I) {
    BlockLayout L;
    GfwRsLayout S;
    memset(&S, 0, sizeof(S));
    S.points = (size_t)gfw_pairs_total(I.pairs(), true);
    S.o_rfirst = L.add(sizeof(int32_t) * ((size_t)I.n_ranges + 1));
    S.o_prange = L.add(sizeof(int32_t) * (size_t)I.n_pairs);
    S.o_pfirst = L.add(sizeof(int32_t) * ((size_t)I.n_pairs + 1));      // the pair timestamps lie between the shared parts: added here, not by gfw_pairs_add
    S.o_pts_us = L.add(sizeof(int64_t) * 2 * (size_t)I.n_pairs);
    S.o_pts = L.add(sizeof(float) * 2 * S.points * 2);
    S.o_tt = L.add(sizeof(double) * (size_t)I.n_track);
    S.o_tq = L.add(sizeof(double) * 4 * (size_t)I.n_track);
    if (I.cand_first) {
        S.o_cfirst = L.add(sizeof(int32_t) * ((size_t)I.n_ranges + 1));
        S.o_cand = L.add(sizeof(double) * (size_t)I.n_candidates);
        S.o_pcfirst = L.add(sizeof(int64_t) * (size_t)I.n_pairs);
        for (int r = 0; r < I.n_ranges; ++r) {
            const int nc = I.cand_first[r + 1] - I.cand_first[r];
            S.pair_costs += (size_t)nc * (size_t)(I.range_first[r + 1] - I.range_first[r]);
            if (I.range_first[r + 1] > I.range_first[r] && nc > S.max_cand) S.max_cand = nc;
        }
    }
    for (int p = 0; p < I.n_pairs; ++p) { const int n = I.pair_first[p + 1] - I.pair_first[p]; if (n > S.max_pair) S.max_pair = n; }
    S.total = L.total;
    return S;
}
// Fills the block at (h, d) and the argument block's input pointers and counts
inline void gfw_rs_fill(const GfwRsLayout &S, const GfwRsInputs &I, char *h, const char *d, GfwRsArgs &A) {
    memcpy(h + S.o_rfirst, I.range_first, sizeof(int32_t) * ((size_t)I.n_ranges + 1));
    int32_t *prange = (int32_t *)(h + S.o_prange);
    for (int r = 0; r < I.n_ranges; ++r)
        for (int p = I.range_first[r]; p < I.range_first[r + 1]; ++p) prange[p] = r;
    A.total = gfw_pairs_fill(S.o_pfirst, S.o_pts, I.pairs(), true, h, d, A.pair_first, A.points);
    if (I.n_pairs) memcpy(h + S.o_pts_us, I.pair_ts_us, sizeof(int64_t) * 2 * (size_t)I.n_pairs);
    double *tt = (double *)(h + S.o_tt);
    for (int i = 0; i < I.n_track; ++i) tt[i] = (double)I.track_ts_us[i] / 1000000.0;
    memcpy(h + S.o_tq, I.track_wxyz, sizeof(double) * 4 * (size_t)I.n_track);
    if (I.cand_first) {
        memcpy(h + S.o_cfirst, I.cand_first, sizeof(int32_t) * ((size_t)I.n_ranges + 1));
        if (I.n_candidates) memcpy(h + S.o_cand, I.candidates, sizeof(double) * (size_t)I.n_candidates);
        int64_t *pc = (int64_t *)(h + S.o_pcfirst), at = 0;
        for (int r = 0; r < I.n_ranges; ++r)
            for (int p = I.range_first[r]; p < I.range_first[r + 1]; ++p) { pc[p] = at; at += I.cand_first[r + 1] - I.cand_first[r]; }
        A.cand_first = (const int32_t *)(d + S.o_cfirst); A.cand = (const double *)(d + S.o_cand); A.pc_first = (const int64_t *)(d + S.o_pcfirst);
    }
    A.range_first = (const int32_t *)(d + S.o_rfirst); A.pair_range = (const int32_t *)(d + S.o_prange); A.pair_ts = (const int64_t *)(d + S.o_pts_us);
    A.track_t = (const double *)(d + S.o_tt); A.track_q = (const double *)(d + S.o_tq);
    A.n_ranges = I.n_ranges; A.n_pairs = I.n_pairs; A.n_track = I.n_track; A.lds_points = S.max_pair;
}
// The call's constants
inline void gfw_rs_constants(int video_w, int video_h, int flow_w, int flow_h, double frame_readout_time_ms, const GfwRsSettings &S, GfwRsArgs &A) {
    A.vw = (float)video_w; A.vh = (float)video_h; A.fw = (float)flow_w; A.fh = (float)flow_h;
    A.flow_h = (double)flow_h; A.readout_s = frame_readout_time_ms / 1000.0;         // rs_sync.rs:81
    A.loss_scale = S.loss_scale; A.hypotheses = S.hypotheses; A.refits = S.refits; A.sweeps = S.sweeps; A.refine = S.refine;
}
// Round `round` of a search: the candidates' count, place and step
inline void gfw_rs_round(const GfwRsSettings &S, int round, GfwRsArgs &A) {
    const int n0 = gfw_rs_round0_count(S.radius_s, S.step_s);
    double step = S.step_s;
    for (int k = 0; k < round; ++k) step = step / 8.0;
    A.mode = round == 0 ? 1 : 2;
    A.n_cand = round == 0 ? n0 : GFW_RS_LATER; A.half = (n0 - 1) / 2;
    A.at = round == 0 ? 0 : n0 + (round - 1) * GFW_RS_LATER;
    A.total_cand = n0 + (S.rounds - 1) * GFW_RS_LATER;
    A.initial = S.initial_delay_s; A.step = step; A.next_step = step / 8.0; A.last = round == S.rounds - 1 ? 1 : 0;
}
