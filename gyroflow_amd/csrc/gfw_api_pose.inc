// gfw_api_pose.inc — part of gfw_api.hip (textually included): gfw_pose_almeida and gfw_pose_draws.  What they check and stage is gfw_pose_host.h's; the pair set's check and staging and the lens gate, shared with the other point-pair calls, gfw_pairs_host.h's.

// Almeida pose estimation of every frame pair of a call (estimate_pose/almeida.rs:23-238; gfw_pose.hip).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_pose_almeida(gfw_ctx *c, const gfw_kernel_params *p, const gfw_pose_almeida_cfg *cfg, const int32_t *pair_first, const float *points_a,
                                const float *points_b, int n_pairs, const int32_t *triples, const int32_t *sample_first, const int32_t *samples,
                                float *quats, double *rotations, int32_t *best, int32_t *round_inliers, float *round_fits, int out_on_device) {
    if (!c || !p || !cfg) { set_error("bad pose arguments (null context / params / configuration)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (cfg->reserved) { set_error("bad pose configuration: the reserved slot must be 0"); return GFW_ERR_INVALID_ARGUMENT; }
    char why[256];
    if (!gfw_pairs_lens_check(*p, cfg->camera_matrix, {cfg->video_width, cfg->video_height, cfg->flow_width, cfg->flow_height}, "pose", "pose estimation", cfg->inlier_angle_deg >= 0.0f,
                              why, sizeof(why), "inlier angle %g", (double)cfg->inlier_angle_deg)) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwPoseInputs I = {pair_first, points_a, points_b, n_pairs, triples, sample_first, samples, cfg->num_iters, cfg->num_samples};
    if (!gfw_pose_check(I, why, sizeof(why))) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_pairs == 0) return GFW_OK;
    if (!quats || !rotations || !best) { set_error("bad pose arguments (a null quats / rotations / best array)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwPoseLayout S = gfw_pose_layout(I);
    if (S.total > ((size_t)1 << 31)) { set_error("the call stages %zu bytes (%d pairs x %d rounds): at most 2 GiB", S.total, n_pairs, cfg->num_iters); return GFW_ERR_INVALID_ARGUMENT; }
    API_TRY(enter_device(c));
    // pairs, points and draws through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    GfwPoseArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->pose_ring.acquire(S.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_pose_fill(S, I, B.h(), B.d(), A);
    gfw_pose_constants(cfg->video_width, cfg->video_height, cfg->flow_width, cfg->flow_height, cfg->inlier_angle_deg, cfg->camera_matrix, A);
    HIP_TRY(B.upload(S.total, c->stream), GFW_ERR_HIP);
    const size_t rounds = (size_t)n_pairs * (size_t)cfg->num_iters, total = (size_t)A.total;
    CallOutputs O(c->d_out, out_on_device);
    const int o_quats = O.add(quats, sizeof(float) * 4 * (size_t)n_pairs);
    const int o_rot = O.add(rotations, sizeof(double) * 9 * (size_t)n_pairs);
    const int o_best = O.add(best, sizeof(int32_t) * 2 * (size_t)n_pairs);
    const int o_counts = O.add(round_inliers, sizeof(int32_t) * rounds);
    const int o_fits = O.add(round_fits, sizeof(float) * 4 * rounds);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    // device work space: what the prepare stage leaves per point, and the rounds' fits and counts where the caller does not ask for them
    BlockLayout W;
    const size_t w_pm = W.add(sizeof(float4) * total), w_rays = W.add(sizeof(float4) * total), w_derivs = W.add(sizeof(float2) * 3 * total);
    const size_t w_fits = W.add(sizeof(float) * 4 * rounds), w_counts = W.add(sizeof(int32_t) * rounds);
    HIP_TRY(c->d_sync_work.ensure(W.total + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    A.pm = (float4 *)(wk + w_pm); A.rays = (float4 *)(wk + w_rays); A.derivs = (float2 *)(wk + w_derivs);
    A.fits = round_fits ? (float *)O.dev(o_fits) : (float *)(wk + w_fits);
    A.counts = round_inliers ? (int32_t *)O.dev(o_counts) : (int32_t *)(wk + w_counts);
    A.quats = (float *)O.dev(o_quats); A.rotations = (double *)O.dev(o_rot); A.best = (int32_t *)O.dev(o_best);
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    HIP_TRY(gfw_launch_pose_prepare(*p, C, A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_pose_fit(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_pose_count(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_pose_pick(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads the slot's device side
    c->last_backend = "pose_almeida";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    return GFW_OK;
}

// The draws of a call (gfw_pose_draws_host): host only, no context
extern "C" int gfw_pose_draws(uint64_t seed, const int32_t *pair_first, int n_pairs, int num_iters, int num_samples, int32_t *triples, const int32_t *sample_first, int32_t *samples) {
    if (!gfw_pose_draws_host(seed, pair_first, n_pairs, num_iters, num_samples, triples, sample_first, samples)) {
        set_error("bad pose draw arguments (a negative count, a null array, a descending pair_first, a pair above %d points, or a sample_first that does not hold num_iters x min(n, num_samples) entries a pair)", GFW_POSE_PAIR_MAX);
        return GFW_ERR_INVALID_ARGUMENT; }
    return GFW_OK;
}
