// gfw_api_sync.inc — part of gfw_api.hip (textually included): the sync searches' entry points — gfw_sync_visual_*, gfw_lowpass_gyro, gfw_sync_gyro_*.  What the visual
// search checks and what they stage is gfw_sync_host.h's and gfw_sync_gyro_host.h's.

// The visual-features sync search (find_offset/visual_features.rs:10-147; gfw_sync.hip).  See include/gfwarp.h for the argument contract.  One body serves both entries:
// `search_mode` < 0 = gfw_sync_visual_costs (the caller's candidates), 0 / 1 = gfw_sync_visual_search (the coarse candidates are made here, the fine ones on the device).
struct SyncOut { double *costs; float *mapped; gfw_sync_result *result; double *coarse_costs, *fine_costs; };
static int sync_visual_impl(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_search *search, const int64_t *pair_ts_us, const int32_t *pair_first,
                            const float *points_a, const float *points_b, int n_pairs, const double *candidates, int n_candidates, int search_mode,
                            double initial_offset_ms, double search_size_ms, double frame_readout_time_ms, double scaled_fps, const SyncOut &out, int out_on_device) {
    if (!c || !p) { set_error("bad sync arguments (null context / params / search, or a negative count)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwPairSet P = {pair_ts_us, pair_first, points_a, points_b, n_pairs};
    int total = 0, max_pair = 0, n_coarse = 0;
    char why[256];
    if (!gfw_sync_check(search, p->flags, P, candidates, n_candidates, search_mode, search_size_ms, scaled_fps, search_mode < 0 ? (const void *)out.costs : (const void *)out.result, total, max_pair, n_coarse, why, sizeof(why))) {
        set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (c->tracks.org_n < 1 && c->tracks.sm_n < 1) { set_error("no quaternion tracks set (gfw_set_quaternion_tracks)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (search_mode < 0 && n_candidates == 0) return GFW_OK;
    API_TRY(enter_device(c));
    // pairs, points and candidates through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    const GfwSyncLayout S = gfw_sync_layout(n_pairs, total, (size_t)n_coarse);
    GfwSyncArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->sync_ring.acquire(S.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_sync_fill(S, pair_ts_us, pair_first, points_a, points_b, n_pairs, search_mode < 0 ? candidates : nullptr, n_coarse, search_mode, initial_offset_ms, search_size_ms,
                  frame_readout_time_ms, B.h(), B.d(), A);
    HIP_TRY(B.upload(S.total, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);
    // device work space: rays, partials of the larger stage, the fine candidates
    const int n_wide = search_mode < 0 ? n_coarse : (n_coarse > GFW_SYNC_FINE ? n_coarse : GFW_SYNC_FINE);
    const size_t rb = sizeof(float4) * 2 * (size_t)total, qb = sizeof(unsigned long long) * (size_t)n_wide * (size_t)(n_pairs ? n_pairs : 1), eb = sizeof(double) * 2 * GFW_SYNC_FINE;
    HIP_TRY(c->d_sync_work.ensure(rb + qb + eb + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    CallOutputs O(c->d_out, out_on_device);
    const int o_result = O.add(out.result, sizeof(gfw_sync_result));
    const int o_costs = O.add(search_mode < 0 ? out.costs : out.coarse_costs, sizeof(double) * (size_t)n_coarse);
    const int o_fine = O.add(out.fine_costs, sizeof(double) * GFW_SYNC_FINE);
    const int o_mapped = O.add(out.mapped, sizeof(float) * 4 * (size_t)total * (size_t)n_coarse);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    gfw_sync_result *d_result = (gfw_sync_result *)O.dev(o_result);
    A.T = c->tracks;
    if (!search->use_sync_offsets) { A.T.off_ts = nullptr; A.T.off_ms = nullptr; A.T.off_n = 0; }      // clear_offsets()
    for (int i = 0; i < 9; ++i) A.F.new_k[i] = search->new_k[i];
    A.F.video_rotation_deg = search->video_rotation_deg;
    A.rays = (float4 *)wk; A.partial = (unsigned long long *)(wk + rb);
    A.mapped = (float *)O.dev(o_mapped);
    A.w = (float)search->width; A.h = (float)search->height;
    A.horizontal = search->horizontal_readout; A.readout_dim = search->horizontal_readout ? search->width : search->height;
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    GfwSyncReduceArgs R;
    memset(&R, 0, sizeof(R));
    R.partial = A.partial; R.candidates = A.candidates; R.costs = (double *)O.dev(o_costs); R.result = d_result; R.fine = (double *)(wk + rb + qb);
    R.n = n_coarse; R.n_pairs = n_pairs; R.column = search_mode == 1 ? 1 : 0; R.stage = 0;
    HIP_TRY(gfw_launch_sync_rays(*p, C, A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_sync_costs(A, n_coarse, max_pair, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_sync_reduce(R, c->stream), GFW_ERR_HIP);
    if (search_mode >= 0) {
        A.candidates = R.fine; A.gate = d_result; A.mapped = nullptr;
        HIP_TRY(gfw_launch_sync_costs(A, GFW_SYNC_FINE, max_pair, c->stream), GFW_ERR_HIP);
        R.candidates = R.fine; R.costs = (double *)O.dev(o_fine); R.n = GFW_SYNC_FINE; R.stage = 1;
        HIP_TRY(gfw_launch_sync_reduce(R, c->stream), GFW_ERR_HIP);
    }
    c->last_backend = search_mode < 0 ? "sync_visual_costs" : "sync_visual_search";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    return GFW_OK;
}
extern "C" int gfw_sync_visual_costs(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_search *search, const int64_t *pair_ts_us, const int32_t *pair_first,
                                     const float *points_a, const float *points_b, int n_pairs, const double *candidates, int n_candidates,
                                     double *costs, float *mapped, int out_on_device) {
    const SyncOut out = {costs, mapped, nullptr, nullptr, nullptr};
    return sync_visual_impl(c, p, search, pair_ts_us, pair_first, points_a, points_b, n_pairs, candidates, n_candidates, -1, 0.0, 0.0, 0.0, 0.0, out, out_on_device);
}
extern "C" int gfw_sync_visual_search(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_search *search, const int64_t *pair_ts_us, const int32_t *pair_first,
                                      const float *points_a, const float *points_b, int n_pairs, int mode, double initial_offset_ms, double search_size_ms,
                                      double frame_readout_time_ms, double scaled_fps, gfw_sync_result *result, double *coarse_costs, double *fine_costs, int out_on_device) {
    const SyncOut out = {nullptr, nullptr, result, coarse_costs, fine_costs};
    return sync_visual_impl(c, p, search, pair_ts_us, pair_first, points_a, points_b, n_pairs, nullptr, 0, mode < 0 ? 2 : mode, initial_offset_ms, search_size_ms,
                            frame_readout_time_ms, scaled_fps, out, out_on_device);
}

// Lowpass::filter_gyro_forward_backward (filtering.rs:46-74) of a gyro triple series, in place (gfw_lowpass_gyro_host).  See include/gfwarp.h.
extern "C" int gfw_lowpass_gyro(double freq, double sample_rate, double *xyz, const uint8_t *has, int n) {
    if (n < 0 || (n && !xyz)) { set_error("bad lowpass arguments (n %d)", n); return GFW_ERR_INVALID_ARGUMENT; }
    return gfw_lowpass_gyro_host(freq, sample_rate, xyz, has, n) ? GFW_OK : GFW_FILTER_NOT_APPLIED;
}

// The gyro-match sync search (find_offset/essential_matrix.rs:52-75, :109-131; gfw_sync_gyro.hip).  See include/gfwarp.h for the argument contract.  One body serves
// both entries: `search` false = gfw_sync_gyro_costs (the caller's candidates), true = gfw_sync_gyro_search (the coarse candidates are made here, the fine ones on the device).
struct GyroSeries { const int32_t *first; const double *data; const uint8_t *has; int total; const char *what; int limit; };
static bool gyro_series_ok(const GyroSeries &s, int n_ranges, bool needs_data = true) {
    if (!s.first || s.total < 0) { set_error("bad sync arguments (%s: a null first array, or a negative length %d)", s.what, s.total); return false; }
    if (s.first[0] < 0) { set_error("range 0: %s first %d is negative", s.what, s.first[0]); return false; }
    for (int r = 0; r < n_ranges; ++r) {
        if (s.first[r + 1] < s.first[r]) { set_error("range %d: %s first descends (%d after %d)", r, s.what, s.first[r + 1], s.first[r]); return false; }
        if (s.first[r + 1] > s.total) { set_error("range %d: %s slice %d .. %d lies outside its array of %d", r, s.what, s.first[r], s.first[r + 1], s.total); return false; }
        if (s.first[r + 1] - s.first[r] > s.limit) { set_error("range %d: %d %s, at most %d", r, s.first[r + 1] - s.first[r], s.what, s.limit); return false; }
    }
    if (needs_data && s.first[n_ranges] > 0 && !s.data) { set_error("bad sync arguments (%d %s without their array)", s.first[n_ranges], s.what); return false; }
    return true;
}
static int sync_gyro_impl(gfw_ctx *c, const GyroSeries &est, const GyroSeries &gyro, int n_ranges, const GyroSeries &cand, bool search,
                          double initial_offset_ms, double search_size_ms, double *costs, gfw_sync_result *results, double *coarse_costs, double *fine_costs, int out_on_device) {
    if (!c || n_ranges < 0) { set_error("bad sync arguments (null context, or a negative range count)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_ranges > GFW_GYRO_RANGES_MAX) { set_error("%d ranges: at most %d in a call", n_ranges, GFW_GYRO_RANGES_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    size_t n_coarse = 0;
    if (search) {
        if (!std::isfinite(initial_offset_ms) || !std::isfinite(search_size_ms) || search_size_ms < 0.0) {
            set_error("bad sync search: initial_offset_ms %g, search_size_ms %g", initial_offset_ms, search_size_ms); return GFW_ERR_INVALID_ARGUMENT; }
        if (search_size_ms * 2.0 > (double)GFW_GYRO_COARSE_MAX) { set_error("a search of %g candidates a range (search_size_ms %g), at most %d", trunc(search_size_ms) * 2.0, search_size_ms, GFW_GYRO_COARSE_MAX); return GFW_ERR_INVALID_ARGUMENT; }
        n_coarse = (size_t)search_size_ms * 2;                              // `search_size as usize * 2` (:55): the cast comes first
        if (n_ranges && !results) { set_error("bad sync arguments (a null result array)"); return GFW_ERR_INVALID_ARGUMENT; }
    } else if (n_ranges && !costs) { set_error("bad sync arguments (a null cost array)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_ranges == 0) return GFW_OK;
    if (!gyro_series_ok(est, n_ranges) || !gyro_series_ok(gyro, n_ranges) || (!search && !gyro_series_ok(cand, n_ranges))) return GFW_ERR_INVALID_ARGUMENT;
    const size_t tot_est = (size_t)est.first[n_ranges] - (size_t)est.first[0], tot_gyro = (size_t)gyro.first[n_ranges] - (size_t)gyro.first[0];
    const size_t tot_cand = search ? n_coarse * (size_t)n_ranges : (size_t)cand.first[n_ranges] - (size_t)cand.first[0];
    const GfwGyroLayout L = gfw_gyro_layout(n_ranges, tot_est, tot_gyro, tot_cand);
    if (L.total > ((size_t)1 << 31)) { set_error("the call stages %zu bytes (%zu estimated samples, %zu gyro samples, %zu candidates): at most 2 GiB", L.total, tot_est, tot_gyro, tot_cand); return GFW_ERR_INVALID_ARGUMENT; }
    if (!search && tot_cand == 0) return GFW_OK;
    API_TRY(enter_device(c));
    // everything through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    GfwGyroArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->gyro_ring.acquire(L.total, c->stream, &B.slot), GFW_ERR_HIP);
    const GfwGyroSeries se = {est.first, est.data, est.has}, sg = {gyro.first, gyro.data, gyro.has};
    const int max_cand = gfw_gyro_fill(L, se, sg, n_ranges, search ? nullptr : cand.first, cand.data, n_coarse, initial_offset_ms, search_size_ms, B.h(), B.d(), A);
    HIP_TRY(B.upload(L.total, c->stream), GFW_ERR_HIP);
    // outputs the caller does not ask for live in the work space.  Caller-given candidates: range r's costs are the caller's entries cand_first[r] ..; the staged
    // ranges count from 0, so the base moves by cand_first[0]
    const size_t fine_n = GFW_GYRO_FINE * (size_t)n_ranges;
    CallOutputs O(c->d_out, out_on_device);
    const int o_results = O.add(results, sizeof(gfw_sync_result) * (size_t)n_ranges);
    const int o_costs = O.add(search ? coarse_costs : costs + cand.first[0], 8 * tot_cand);
    const int o_fine = O.add(fine_costs, 8 * fine_n);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    gfw_sync_result *d_results = (gfw_sync_result *)O.dev(o_results);
    double *d_costs = (double *)O.dev(o_costs), *d_fine_costs = (double *)O.dev(o_fine);
    HIP_TRY(c->d_sync_work.ensure(8 * fine_n * 2 + 8 * tot_cand + 16), GFW_ERR_HIP);
    double *wk = (double *)c->d_sync_work.ptr;
    A.costs = d_costs ? d_costs : wk + 2 * fine_n; A.stage = 0;
    HIP_TRY(gfw_launch_gyro_costs(A, n_ranges, max_cand, c->stream), GFW_ERR_HIP);
    if (search) {
        GfwGyroPickArgs R;
        memset(&R, 0, sizeof(R));
        R.ranges = A.ranges; R.candidates = A.candidates; R.costs = A.costs; R.results = d_results; R.fine = wk; R.stage = 0;
        HIP_TRY(gfw_launch_gyro_pick(R, n_ranges, c->stream), GFW_ERR_HIP);
        A.candidates = wk; A.costs = d_fine_costs ? d_fine_costs : wk + fine_n; A.gate = d_results; A.stage = 1;
        HIP_TRY(gfw_launch_gyro_costs(A, n_ranges, GFW_GYRO_FINE, c->stream), GFW_ERR_HIP);
        R.candidates = wk; R.costs = A.costs; R.fine_costs = d_fine_costs; R.stage = 1;
        HIP_TRY(gfw_launch_gyro_pick(R, n_ranges, c->stream), GFW_ERR_HIP);
    }
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads the slot's device side
    c->last_backend = search ? "sync_gyro_search" : "sync_gyro_costs";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    return GFW_OK;
}
extern "C" int gfw_sync_gyro_costs(gfw_ctx *c, const int32_t *est_first, const double *est, const uint8_t *est_has, int n_est,
                                   const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has, int n_gyro, int n_ranges,
                                   const int32_t *cand_first, const double *candidates, int n_candidates, double *costs, int out_on_device) {
    const GyroSeries e = {est_first, est, est_has, n_est, "estimated samples", GFW_GYRO_EST_MAX}, g = {gyro_first, gyro, gyro_has, n_gyro, "gyro samples", GFW_GYRO_SAMPLES_MAX};
    const GyroSeries k = {cand_first, candidates, nullptr, n_candidates, "candidates", GFW_GYRO_COARSE_MAX};
    return sync_gyro_impl(c, e, g, n_ranges, k, false, 0.0, 0.0, costs, nullptr, nullptr, nullptr, out_on_device);
}
extern "C" int gfw_sync_gyro_search(gfw_ctx *c, const int32_t *est_first, const double *est, const uint8_t *est_has, int n_est,
                                    const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has, int n_gyro, int n_ranges,
                                    double initial_offset_ms, double search_size_ms, gfw_sync_result *results, double *coarse_costs, double *fine_costs, int out_on_device) {
    const GyroSeries e = {est_first, est, est_has, n_est, "estimated samples", GFW_GYRO_EST_MAX}, g = {gyro_first, gyro, gyro_has, n_gyro, "gyro samples", GFW_GYRO_SAMPLES_MAX};
    const GyroSeries k = {nullptr, nullptr, nullptr, 0, "candidates", GFW_GYRO_COARSE_MAX};
    return sync_gyro_impl(c, e, g, n_ranges, k, true, initial_offset_ms, search_size_ms, nullptr, results, coarse_costs, fine_costs, out_on_device);
}
