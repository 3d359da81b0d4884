// gfw_api_varref.inc — part of gfw_api.hip (textually included behind gfw_api_dis.inc): gfw_flow_dis_refined.  What it checks and sizes is gfw_varref_host.h's on
// top of gfw_dis_host.h's; the sequence, the staging ring and the outputs are gfw_flow_dis's own (flow_dis_run).

// gfw_flow_dis with the variational refinement of every level's field (gfw_varref.hip).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_flow_dis_refined(gfw_ctx *c, const gfw_flow_dis_cfg *cfg, const gfw_flow_varref_cfg *ref, const void *frames, int frames_on_device, int n_frames,
                                    const int32_t *pair_frames, int n_pairs, float *grid_points, int32_t *grid_counts, float *flow, int32_t *out_pair_first,
                                    float *points_a, float *points_b, int out_on_device) {
    if (!c || !cfg || !ref) { set_error("bad refined DIS flow arguments (null context / configuration)"); return GFW_ERR_INVALID_ARGUMENT; }
    const GfwDisInputs I = {cfg->width, cfg->height, cfg->stride, cfg->finest_scale, cfg->variational_iters, cfg->reserved, frames, frames_on_device, n_frames, pair_frames, n_pairs};
    const GfwVarrefInputs V = {ref->fixed_point_iters, ref->sor_iters, ref->alpha, ref->delta, ref->gamma, ref->omega, {ref->reserved[0], ref->reserved[1]}};
    char why[384];
    if (!gfw_varref_check(I, V, why, sizeof(why))) { set_error("%s", why); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_pairs == 0) return GFW_OK;
    return flow_dis_run(c, I, &V, "flow_dis_refined", grid_points, grid_counts, flow, out_pair_first, points_a, points_b, out_on_device);
}
