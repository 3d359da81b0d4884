// gfw_api_corners.inc — part of gfw_api.hip (textually included): gfw_corners_shi_tomasi.  What it checks, sizes and stages is gfw_corners_host.h's.

// Shi-Tomasi corner detection of every frame of a call (optical_flow/opencv_pyrlk.rs:25-42; gfw_corners.hip).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_corners_shi_tomasi(gfw_ctx *c, const gfw_corners_cfg *cfg, const void *frames, int frames_on_device, int n_frames,
                                      float *corners, float *scores, int32_t *counts, int32_t *feat_first, float *features, int out_on_device) {
    if (!c || !cfg) { set_error("bad corners arguments (null context / configuration)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwCornersInputs I = {cfg->width, cfg->height, cfg->stride, cfg->max_corners, cfg->quality, cfg->min_distance, cfg->max_workspace_mb, cfg->reserved,
                                frames, frames_on_device, n_frames, corners, counts, feat_first, features};
    char why[256];
    if (!gfw_corners_check(I, why, sizeof(why))) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_frames == 0) return GFW_OK;
    const GfwCornersPlan P = gfw_corners_plan(I);
    API_TRY(enter_device(c));
    const size_t room = (size_t)n_frames * (size_t)cfg->max_corners;
    // device work space: the candidate lists of one batch, the packed corners of a call with host outputs
    BlockLayout W;
    const size_t w_cand = W.add(P.cand_bytes), w_feat = W.add(features && !out_on_device ? sizeof(float) * 2 * room : 0);
    HIP_TRY(c->d_sync_work.ensure(W.total + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    // the zeroed maxima and counts and host frames through pinned memory in one copy: it is enqueued, the caller's frames are free on return
    GfwCornersArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->corners_ring.acquire(P.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_corners_fill(P, I, B.h(), (char *)B.slot->d.ptr, (unsigned long long *)(wk + w_cand), A);
    HIP_TRY(B.upload(P.total, c->stream), GFW_ERR_HIP);
    CallOutputs O(c->d_out, out_on_device);
    const int o_corners = O.add(corners, sizeof(float) * 2 * room), o_scores = O.add(scores, sizeof(float) * room), o_counts = O.add(counts, sizeof(int32_t) * (size_t)n_frames);
    const int o_first = O.add(feat_first, sizeof(int32_t) * ((size_t)n_frames + 1));
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    A.corners = (float *)O.dev(o_corners); A.scores = (float *)O.dev(o_scores); A.counts = (int32_t *)O.dev(o_counts); A.feat_first = (int32_t *)O.dev(o_first);
    A.features = features ? (out_on_device ? features : (float *)(wk + w_feat)) : nullptr;
    for (int b = 0; b < P.n_batches; ++b) {                                 // the lists of a batch are the next batch's: in turn on the stream
        gfw_corners_batch(P, b, A);
        HIP_TRY(gfw_launch_corners_eig(A, c->stream), GFW_ERR_HIP);
        HIP_TRY(gfw_launch_corners_pick(A, c->stream), GFW_ERR_HIP);
    }
    HIP_TRY(gfw_launch_corners_scan(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_corners_pack(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads or writes the slot's device side
    c->last_backend = "corners_shi_tomasi";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    if (!out_on_device && features) {                                       // (finish has waited) only the kept corners go to the caller's array
        const size_t kept = sizeof(float) * 2 * (size_t)feat_first[n_frames];
        if (kept) {
            HIP_TRY(hipMemcpyAsync(features, A.features, kept, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
            HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
        }
    }
    return GFW_OK;
}
