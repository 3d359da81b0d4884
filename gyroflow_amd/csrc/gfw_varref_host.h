// gfw_varref_host.h — host only: what gfw_flow_dis_refined checks and sizes on top of gfw_dis_host.h for the kernels of gfw_varref.hip.  Included behind gfw_dis.h,
// gfw_dis_host.h and gfw_varref.h by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit sees it and it calls nothing of HIP.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

// The refinement's configuration of one call (include/gfwarp.h: gfw_flow_varref_cfg)
struct GfwVarrefInputs { int fixed_point_iters, sor_iters; float alpha, delta, gamma, omega; int reserved[2]; };

// The refinement's device work space behind the DIS plan's: GFW_VARREF_PLANES planes of one float per pixel and pair of the finest level — the largest a call
// refines; the coarser levels use the front of each plane.  All pairs of a level go through every launch; dealing them into batches that fit the cache is not built.
struct GfwVarrefPlan {
    size_t plane_bytes, plane_at[GFW_VARREF_PLANES], work_bytes;
    int levels, launches;                                                    // levels refined, and the launches the refinement adds to the call
};
inline GfwVarrefPlan gfw_varref_plan(const GfwDisInputs &I, const GfwDisPlan &D, const GfwVarrefInputs &V) {
    GfwVarrefPlan P;
    memset(&P, 0, sizeof(P));
    if (V.fixed_point_iters <= 0 || I.n_pairs <= 0) return P;
    P.plane_bytes = sizeof(float) * (size_t)I.n_pairs * (size_t)D.lw[I.finest] * (size_t)D.lh[I.finest];
    BlockLayout W;
    for (int k = 0; k < GFW_VARREF_PLANES; ++k) P.plane_at[k] = W.add(P.plane_bytes);
    P.work_bytes = W.total;
    P.levels = D.coarsest - I.finest + 1;
    P.launches = P.levels * gfw_varref_launches(V.fixed_point_iters, V.sor_iters);
    return P;
}
// -> true, or false with the reason in `err`: the refinement's own configuration first, then everything gfw_flow_dis checks, then the two work spaces together
inline bool gfw_varref_check(const GfwDisInputs &I, const GfwVarrefInputs &V, char *err, size_t cap) {
    if (I.variational_iters) {
        snprintf(err, cap, "bad refined DIS flow configuration: variational_iters %d in gfw_flow_dis_cfg beside fixed_point_iters %d in gfw_flow_varref_cfg "
                 "(the count lives in gfw_flow_varref_cfg: variational_iters must be 0)", I.variational_iters, V.fixed_point_iters); return false; }
    if (V.reserved[0] || V.reserved[1]) { snprintf(err, cap, "bad refinement configuration: the reserved slots must be 0"); return false; }
    if (V.fixed_point_iters < 0 || V.fixed_point_iters > GFW_VARREF_ITERS_MAX) {
        snprintf(err, cap, "bad refinement configuration: fixed_point_iters %d (0 to %d)", V.fixed_point_iters, GFW_VARREF_ITERS_MAX); return false; }
    if (V.sor_iters < 1 || V.sor_iters > GFW_VARREF_ITERS_MAX) { snprintf(err, cap, "bad refinement configuration: sor_iters %d (1 to %d)", V.sor_iters, GFW_VARREF_ITERS_MAX); return false; }
    if (!isfinite(V.alpha) || !(V.alpha > 0.0f)) { snprintf(err, cap, "bad refinement configuration: alpha %g (finite and above 0)", (double)V.alpha); return false; }
    if (!isfinite(V.delta) || !(V.delta > 0.0f)) { snprintf(err, cap, "bad refinement configuration: delta %g (finite and above 0)", (double)V.delta); return false; }
    if (!isfinite(V.gamma) || !(V.gamma > 0.0f)) { snprintf(err, cap, "bad refinement configuration: gamma %g (finite and above 0)", (double)V.gamma); return false; }
    if (!isfinite(V.omega) || !(V.omega > 0.0f) || !(V.omega < 2.0f)) { snprintf(err, cap, "bad refinement configuration: omega %g (between 0 and 2, both excluded)", (double)V.omega); return false; }
    if (!gfw_dis_check(I, err, cap)) return false;
    if (I.n_pairs == 0) return true;
    const GfwDisPlan D = gfw_dis_plan(I);
    const GfwVarrefPlan P = gfw_varref_plan(I, D, V);
    if (D.work_bytes + P.work_bytes > GFW_DIS_WORK_MAX) {
        snprintf(err, cap, "the call needs %zu bytes of device work space (%d pairs, %d frames of %d x %d at the finest scale %d, %zu of them the refinement's): at most 16 GiB",
                 D.work_bytes + P.work_bytes, I.n_pairs, I.n_frames, I.width, I.height, I.finest, P.work_bytes); return false; }
    return true;
}
// The block of level `l`: the level's images and field as gfw_dis_fill (and the entry point, for the finest field) left them in A, the planes in the work space at `work`
inline GfwVarrefArgs gfw_varref_level(const GfwVarrefPlan &P, const GfwVarrefInputs &V, const GfwDisArgs &A, int l, char *work) {
    GfwVarrefArgs R;
    memset(&R, 0, sizeof(R));
    R.base = A.lv[l].base; R.frame_bytes = A.lv[l].frame_bytes; R.w = A.lv[l].w; R.h = A.lv[l].h; R.stride = A.lv[l].stride; R.n_pairs = A.n_pairs;
    R.pair_frames = A.pair_frames; R.U = A.dense[l];
    for (int k = 0; k < GFW_VARREF_PLANES; ++k) R.plane[k] = (float *)(work + P.plane_at[k]);
    R.alpha = V.alpha; R.delta = V.delta; R.gamma = V.gamma; R.omega = V.omega;
    return R;
}
