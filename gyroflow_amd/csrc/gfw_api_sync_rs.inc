// gfw_api_sync_rs.inc — part of gfw_api.hip (textually included): gfw_sync_rs_costs and gfw_sync_rs_search.  What they check and stage is gfw_sync_rs_host.h's; the pair set's check and staging and the lens gate, shared with the other point-pair calls, gfw_pairs_host.h's.

// The rs-sync offset search (find_offset/rs_sync.rs, offset method 2; gfw_sync_rs.hip).  See include/gfwarp.h for the argument contract.  One body serves both
// entries: `S.search` false = gfw_sync_rs_costs (the caller's candidates: prepare, cost, sum), true = gfw_sync_rs_search (prepare, then cost and pick per round).
static int sync_rs_impl(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_rs_cfg *cfg, const GfwRsInputs &I, GfwRsSettings S, double *costs,
                        gfw_sync_result *results, double *round_candidates, double *round_costs, int out_on_device) {
    if (!c || !p || !cfg) { set_error("bad rs-sync arguments (null context / params / configuration)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2]) { set_error("bad rs-sync configuration: the reserved slots must be 0"); return GFW_ERR_INVALID_ARGUMENT; }
    char why[256];
    if (!gfw_pairs_lens_check(*p, cfg->camera_matrix, {cfg->video_width, cfg->video_height, cfg->flow_width, cfg->flow_height}, "rs-sync", "the rs-sync search", std::isfinite(cfg->frame_readout_time_ms),
                              why, sizeof(why), "frame_readout_time_ms %g", cfg->frame_readout_time_ms)) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    S.step_s = cfg->step_s; S.loss_scale = cfg->loss_scale; S.rounds = cfg->rounds; S.refine = cfg->refine;
    S.hypotheses = cfg->hypotheses; S.refits = cfg->refits; S.sweeps = cfg->jacobi_sweeps;
    if (!gfw_rs_check(I, S, why, sizeof(why))) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (I.n_ranges == 0) return GFW_OK;
    if (S.search ? !results : (I.n_candidates && !costs)) { set_error("bad rs-sync arguments (a null %s array)", S.search ? "result" : "cost"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!S.search && I.n_candidates == 0) return GFW_OK;
    const GfwRsLayout L = gfw_rs_layout(I);
    if (L.total > ((size_t)1 << 31)) { set_error("the call stages %zu bytes (%d pairs, %zu points, %d track samples): at most 2 GiB", L.total, I.n_pairs, L.points, I.n_track); return GFW_ERR_INVALID_ARGUMENT; }
    API_TRY(enter_device(c));
    // everything through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    GfwRsArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->rs_ring.acquire(L.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_rs_fill(L, I, B.h(), B.d(), A);
    gfw_rs_constants(cfg->video_width, cfg->video_height, cfg->flow_width, cfg->flow_height, cfg->frame_readout_time_ms, S, A);
    HIP_TRY(B.upload(L.total, c->stream), GFW_ERR_HIP);
    const int n0 = S.search ? gfw_rs_round0_count(S.radius_s, S.step_s) : 0;
    const size_t row = S.search ? (size_t)n0 + (size_t)(S.rounds - 1) * GFW_RS_LATER : 0, rows = row * (size_t)I.n_ranges;
    CallOutputs O(c->d_out, out_on_device);
    const int o_results = O.add(results, sizeof(gfw_sync_result) * (size_t)I.n_ranges);
    const int o_costs = O.add(costs, sizeof(double) * (size_t)I.n_candidates);
    const int o_rcand = O.add(round_candidates, sizeof(double) * rows);
    const int o_rcost = O.add(round_costs, sizeof(double) * rows);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    // device work space: what the prepare stage leaves per point and side, the costs per (pair, candidate), and the rounds' rows where the caller does not ask for them
    BlockLayout W;
    const size_t w_prep = W.add(sizeof(double) * 8 * L.points);
    const size_t w_pc = W.add(sizeof(double) * (S.search ? (size_t)I.n_pairs * (size_t)(n0 > GFW_RS_LATER ? n0 : GFW_RS_LATER) : L.pair_costs));
    const size_t w_cand = W.add(sizeof(double) * rows), w_sums = W.add(sizeof(double) * rows);
    HIP_TRY(c->d_sync_work.ensure(W.total + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    A.prep = (double *)(wk + w_prep); A.pair_costs = (double *)(wk + w_pc);
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    HIP_TRY(gfw_launch_rs_prepare(*p, C, A, c->stream), GFW_ERR_HIP);
    if (S.search) {
        A.cand_all = round_candidates ? (double *)O.dev(o_rcand) : (double *)(wk + w_cand);
        A.sums_all = round_costs ? (double *)O.dev(o_rcost) : (double *)(wk + w_sums);
        A.results = (gfw_sync_result *)O.dev(o_results);
        for (int round = 0; round < S.rounds; ++round) {
            gfw_rs_round(S, round, A);
            HIP_TRY(gfw_launch_rs_costs(A, A.n_cand, c->stream), GFW_ERR_HIP);
            HIP_TRY(gfw_launch_rs_pick(A, c->stream), GFW_ERR_HIP);
        }
    } else {
        A.mode = 0; A.sums_all = (double *)O.dev(o_costs);
        HIP_TRY(gfw_launch_rs_costs(A, L.max_cand, c->stream), GFW_ERR_HIP);
        HIP_TRY(gfw_launch_rs_pick(A, c->stream), GFW_ERR_HIP);
    }
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads the slot's device side
    c->last_backend = S.search ? "sync_rs_search" : "sync_rs_costs";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    return GFW_OK;
}
extern "C" int gfw_sync_rs_costs(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_rs_cfg *cfg, const int32_t *range_first, int n_ranges, const int64_t *pair_ts_us,
                                 const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs, const int64_t *track_ts_us, const double *track_wxyz,
                                 int n_track, const int32_t *cand_first, const double *candidates, int n_candidates, double *costs, int out_on_device) {
    const GfwRsInputs I = {range_first, n_ranges, pair_ts_us, pair_first, points_a, points_b, n_pairs, track_ts_us, track_wxyz, n_track, cand_first, candidates, n_candidates};
    return sync_rs_impl(c, p, cfg, I, GfwRsSettings{}, costs, nullptr, nullptr, nullptr, out_on_device);
}
extern "C" int gfw_sync_rs_search(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_rs_cfg *cfg, const int32_t *range_first, int n_ranges, const int64_t *pair_ts_us,
                                  const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs, const int64_t *track_ts_us, const double *track_wxyz,
                                  int n_track, double initial_delay_s, double radius_s, gfw_sync_result *results, double *round_candidates, double *round_costs,
                                  int out_on_device) {
    const GfwRsInputs I = {range_first, n_ranges, pair_ts_us, pair_first, points_a, points_b, n_pairs, track_ts_us, track_wxyz, n_track, nullptr, nullptr, 0};
    GfwRsSettings S = {};
    S.search = true; S.initial_delay_s = initial_delay_s; S.radius_s = radius_s;
    return sync_rs_impl(c, p, cfg, I, S, nullptr, results, round_candidates, round_costs, out_on_device);
}
