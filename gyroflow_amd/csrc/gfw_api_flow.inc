// gfw_api_flow.inc — part of gfw_api.hip (textually included): gfw_flow_pyrlk.  What it checks, sizes and stages is gfw_flow_host.h's.

// Pyramidal Lucas-Kanade optical flow of every frame pair of a call (optical_flow/opencv_pyrlk.rs:63-119; gfw_flow.hip).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_flow_pyrlk(gfw_ctx *c, const gfw_flow_pyrlk_cfg *cfg, const void *frames, int frames_on_device, int n_frames, const int32_t *pair_frames, int n_pairs,
                              const int32_t *feat_first, const float *features, float *next, uint8_t *status, int32_t *iters, float *grid_points, int32_t *grid_counts,
                              int32_t *out_pair_first, float *points_a, float *points_b, int out_on_device) {
    if (!c || !cfg) { set_error("bad flow arguments (null context / configuration)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwFlowInputs I = {cfg->width, cfg->height, cfg->stride, cfg->point_mode, cfg->reserved, frames, frames_on_device, n_frames, pair_frames, n_pairs, feat_first, features};
    char why[256];
    if (!gfw_flow_check(I, why, sizeof(why))) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_pairs == 0) return GFW_OK;
    if (!next || !status || !out_pair_first || !points_a || !points_b) { set_error("bad flow arguments (a null next / status / out_pair_first / points_a / points_b array)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwFlowPlan P = gfw_flow_plan(I);
    API_TRY(enter_device(c));
    const size_t raw = (size_t)P.raw_total, nodes = (size_t)P.grid.nodes * (size_t)n_frames;
    const bool grid = cfg->point_mode == GFW_FLOW_MODE_GRID;
    // device work space: the pyramid, the grid points where the caller does not ask for them, the compacted points of a call with host outputs
    BlockLayout W;
    const size_t w_pyr = W.add(P.pyramid_bytes);
    const size_t w_gp = W.add(grid && !grid_points ? sizeof(float) * 2 * nodes : 0), w_gc = W.add(grid && !grid_counts ? sizeof(int32_t) * (size_t)n_frames : 0);
    const size_t w_pa = W.add(out_on_device ? 0 : sizeof(float) * 2 * raw), w_pb = W.add(out_on_device ? 0 : sizeof(float) * 2 * raw);
    HIP_TRY(c->d_sync_work.ensure(W.total + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    // pairs, features, host frames and the zeroed kept counts through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    GfwFlowArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->flow_ring.acquire(P.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_flow_fill(P, I, B.h(), (char *)B.slot->d.ptr, (const uint8_t *)(wk + w_pyr), A);
    HIP_TRY(B.upload(P.total, c->stream), GFW_ERR_HIP);
    CallOutputs O(c->d_out, out_on_device);
    const int o_next = O.add(next, sizeof(float) * 2 * raw), o_status = O.add(status, raw), o_iters = O.add(iters, sizeof(int32_t) * 4 * raw);
    const int o_gp = O.add(grid ? grid_points : nullptr, sizeof(float) * 2 * nodes), o_gc = O.add(grid ? grid_counts : nullptr, sizeof(int32_t) * (size_t)n_frames);
    const int o_first = O.add(out_pair_first, sizeof(int32_t) * ((size_t)n_pairs + 1));
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    A.next = (float *)O.dev(o_next); A.status = (uint8_t *)O.dev(o_status); A.iters = (int32_t *)O.dev(o_iters);
    A.grid_points = grid ? (grid_points ? (float *)O.dev(o_gp) : (float *)(wk + w_gp)) : nullptr;
    A.grid_counts = grid ? (grid_counts ? (int32_t *)O.dev(o_gc) : (int32_t *)(wk + w_gc)) : nullptr;
    A.out_pair_first = (int32_t *)O.dev(o_first);
    A.points_a = out_on_device ? points_a : (float *)(wk + w_pa); A.points_b = out_on_device ? points_b : (float *)(wk + w_pb);
    for (int l = 1; l <= P.top; ++l) HIP_TRY(gfw_launch_flow_pyramid(A, l, (uint8_t *)(wk + w_pyr + P.level_at[l]), c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_flow_grid(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_flow_track(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_flow_scan(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_flow_compact(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads or writes the slot's device side
    c->last_backend = "flow_pyrlk";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    if (!out_on_device) {                                                   // (finish has waited) only the kept points go to the caller's arrays
        const size_t kept = sizeof(float) * 2 * (size_t)out_pair_first[n_pairs];
        if (kept) {
            HIP_TRY(hipMemcpyAsync(points_a, A.points_a, kept, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
            HIP_TRY(hipMemcpyAsync(points_b, A.points_b, kept, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
            HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
        }
    }
    return GFW_OK;
}
