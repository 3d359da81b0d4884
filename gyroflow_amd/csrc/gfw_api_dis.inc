// gfw_api_dis.inc — part of gfw_api.hip (textually included): gfw_flow_dis, and the sequence it shares with gfw_flow_dis_refined (gfw_api_varref.inc).  What it
// checks, sizes and stages is gfw_dis_host.h's.

// The call behind its check: staging, the launches of gfw_dis.h and — where V asks for fixed-point iterations — the refinement launches of gfw_varref.h behind
// each level's dense field, the outputs.  V = nullptr is gfw_flow_dis.
static int flow_dis_run(gfw_ctx *c, const GfwDisInputs &I, const GfwVarrefInputs *V, const char *backend, float *grid_points, int32_t *grid_counts, float *flow,
                        int32_t *out_pair_first, float *points_a, float *points_b, int out_on_device) {
    const int n_frames = I.n_frames, n_pairs = I.n_pairs;
    if (!out_pair_first || !points_a || !points_b) { set_error("bad DIS flow arguments (a null out_pair_first / points_a / points_b array)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwDisPlan P = gfw_dis_plan(I);
    const GfwVarrefPlan VP = V ? gfw_varref_plan(I, P, *V) : GfwVarrefPlan{};
    API_TRY(enter_device(c));
    const size_t room = (size_t)P.points_max, nodes = (size_t)P.grid.nodes * (size_t)n_frames;
    // device work space: the plan's, the grid points where the caller does not ask for them, the points of a call with host outputs
    BlockLayout W;
    const size_t w_plan = W.add(P.work_bytes), w_ref = W.add(VP.work_bytes);
    const size_t w_gp = W.add(grid_points ? 0 : sizeof(float) * 2 * nodes), w_gc = W.add(grid_counts ? 0 : sizeof(int32_t) * (size_t)n_frames);
    const size_t w_pa = W.add(out_on_device ? 0 : sizeof(float) * 2 * room), w_pb = W.add(out_on_device ? 0 : sizeof(float) * 2 * room);
    HIP_TRY(c->d_sync_work.ensure(W.total + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    // pairs and host frames through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    GfwDisArgs A;
    GfwFlowArgs G;
    memset(&A, 0, sizeof(A));
    memset(&G, 0, sizeof(G));
    StagedBlock B;
    HIP_TRY(c->dis_ring.acquire(P.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_dis_fill(P, I, B.h(), (char *)B.slot->d.ptr, wk + w_plan, A, G);
    HIP_TRY(B.upload(P.total, c->stream), GFW_ERR_HIP);
    CallOutputs O(c->d_out, out_on_device);
    const int o_gp = O.add(grid_points, sizeof(float) * 2 * nodes), o_gc = O.add(grid_counts, sizeof(int32_t) * (size_t)n_frames);
    const int o_flow = O.add(flow, P.dense_bytes[I.finest]), o_first = O.add(out_pair_first, sizeof(int32_t) * ((size_t)n_pairs + 1));
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    G.grid_points = grid_points ? (float *)O.dev(o_gp) : (float *)(wk + w_gp);
    G.grid_counts = grid_counts ? (int32_t *)O.dev(o_gc) : (int32_t *)(wk + w_gc);
    A.grid_points = G.grid_points; A.grid_counts = G.grid_counts;
    if (flow) A.dense[I.finest] = (float *)O.dev(o_flow);
    A.out_pair_first = (int32_t *)O.dev(o_first);
    A.points_a = out_on_device ? points_a : (float *)(wk + w_pa); A.points_b = out_on_device ? points_b : (float *)(wk + w_pb);
    for (int l = 1; l <= P.coarsest; ++l) HIP_TRY(gfw_launch_dis_pyramid(A, l, (uint8_t *)(wk + w_plan + P.level_at[l]), c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_flow_grid(G, c->stream), GFW_ERR_HIP);
    for (int l = P.coarsest; l >= I.finest; --l) {
        for (int pass = 0; pass < 3; ++pass) HIP_TRY(gfw_launch_dis_pass(A, l, pass, c->stream), GFW_ERR_HIP);
        HIP_TRY(gfw_launch_dis_dense(A, l, c->stream), GFW_ERR_HIP);
        if (!VP.launches) continue;
        const GfwVarrefArgs R = gfw_varref_level(VP, *V, A, l, wk + w_ref);    // the level's field is refined in place before the next finer level reads it
        HIP_TRY(gfw_launch_varref_prepare(R, c->stream), GFW_ERR_HIP);
        for (int fp = 0; fp < V->fixed_point_iters; ++fp) {
            HIP_TRY(gfw_launch_varref_coeff(R, c->stream), GFW_ERR_HIP);
            for (int it = 0; it < V->sor_iters; ++it)
                for (int colour = 0; colour < 2; ++colour) HIP_TRY(gfw_launch_varref_sor(R, colour, c->stream), GFW_ERR_HIP);
        }
        HIP_TRY(gfw_launch_varref_apply(R, c->stream), GFW_ERR_HIP);
    }
    HIP_TRY(gfw_launch_dis_scan(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_dis_nodes(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads the slot's device side
    c->last_backend = backend;
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    if (!out_on_device) {                                                   // (finish has waited) only the returned points go to the caller's arrays
        const size_t kept = sizeof(float) * 2 * (size_t)out_pair_first[n_pairs];
        if (kept) {
            HIP_TRY(hipMemcpyAsync(points_a, A.points_a, kept, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
            HIP_TRY(hipMemcpyAsync(points_b, A.points_b, kept, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
            HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
        }
    }
    return GFW_OK;
}

// DIS dense optical flow of every frame pair of a call, sampled at the grid points (optical_flow/opencv_dis.rs; gfw_dis.hip).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_flow_dis(gfw_ctx *c, const gfw_flow_dis_cfg *cfg, const void *frames, int frames_on_device, int n_frames, const int32_t *pair_frames, int n_pairs,
                            float *grid_points, int32_t *grid_counts, float *flow, int32_t *out_pair_first, float *points_a, float *points_b, int out_on_device) {
    if (!c || !cfg) { set_error("bad DIS flow arguments (null context / configuration)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwDisInputs I = {cfg->width, cfg->height, cfg->stride, cfg->finest_scale, cfg->variational_iters, cfg->reserved, frames, frames_on_device, n_frames, pair_frames, n_pairs};
    char why[256];
    if (!gfw_dis_check(I, why, sizeof(why))) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_pairs == 0) return GFW_OK;
    return flow_dis_run(c, I, nullptr, "flow_dis", grid_points, grid_counts, flow, out_pair_first, points_a, points_b, out_on_device);
}
