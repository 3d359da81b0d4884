// emu_varref_driver.inc — TEST INFRASTRUCTURE: launches of gfw_flow_dis_refined's kernels on the fibers — those of gfw_dis.hip and the grid kernel of gfw_flow.hip
// through emu_dis_driver.inc (included: its bodies, its guarded mappings and gfw_emu_dis itself, the unrefined call), those of gfw_varref.hip here — in the order
// flow_dis_run (gfw_api_dis.inc) enqueues them, over what gfw_varref_check / gfw_varref_plan / gfw_varref_level (the entry point's own host code,
// gfw_varref_host.h) make of the caller's arrays.  Every plane of the refinement's work space is a mapping of its own between two inaccessible pages, like the
// arrays of the DIS plan.  `launches` receives the number of grids run.
#include "emu_dis_driver.inc"
#include "../../gyroflow_amd/csrc/gfw_varref_host.h"

static GfwVarrefArgs emu_vR; static int emu_vcolour;
static void emu_varref_prepare_body() { emu_dis_unfold(); gfw_varref_prepare_kernel(emu_vR); }
static void emu_varref_coeff_body() { emu_dis_unfold(); gfw_varref_coeff_kernel(emu_vR); }
static void emu_varref_sor_body() { emu_dis_unfold(); gfw_varref_sor_kernel(emu_vR, emu_vcolour); }
static void emu_varref_apply_body() { emu_dis_unfold(); gfw_varref_apply_kernel(emu_vR); }
static int emu_vlaunches;
static int emu_varref_run(int grid, void (*body)()) { ++emu_vlaunches; return emu::run_grid(grid, body); }

extern "C" int gfw_emu_varref(int width, int height, int stride, int finest, int variational_iters, int reserved, const int32_t *ref_ints4, const float *ref_floats4,
                              const void *frames, int n_frames, const int32_t *pair_frames, int n_pairs, float *grid_points, int32_t *grid_counts, float *flow,
                              int32_t *out_pair_first, float *points_a, float *points_b, int guard, int32_t *launches, char *why, size_t why_cap) {
    const GfwDisInputs I = {width, height, stride, finest, variational_iters, reserved, frames, 1, n_frames, pair_frames, n_pairs};
    const GfwVarrefInputs V = {ref_ints4[0], ref_ints4[1], ref_floats4[0], ref_floats4[1], ref_floats4[2], ref_floats4[3], {ref_ints4[2], ref_ints4[3]}};
    emu_vlaunches = 0;
    if (!gfw_varref_check(I, V, why, why_cap)) return -1;
    if (n_pairs == 0) return 0;
    if (!out_pair_first || !points_a || !points_b) { snprintf(why, why_cap, "bad DIS flow arguments (a null out_pair_first / points_a / points_b array)"); return -1; }
    const GfwDisPlan P = gfw_dis_plan(I);
    const GfwVarrefPlan VP = gfw_varref_plan(I, P, V);
    std::vector<uint64_t> block(P.total / 8 + 1), work(guard ? 1 : P.work_bytes / 8 + 1), vwork(guard ? 1 : VP.work_bytes / 8 + 1);
    char *h = (char *)block.data();
    GfwDisArgs &A = emu_dA; GfwFlowArgs &G = emu_dG;
    memset(&A, 0, sizeof(A)); memset(&G, 0, sizeof(G));
    gfw_dis_fill(P, I, h, h, (char *)work.data(), A, G);
    EmuDisGuarded M;
    float *plane[GFW_VARREF_PLANES] = {};
    if (guard) {
        for (int l = 1; l <= P.coarsest; ++l) { if (!(A.lv[l].base = M.get((size_t)n_frames * P.lw[l] * P.lh[l], guard == 1))) return -5; }
        for (int l = finest; l <= P.coarsest; ++l) { if (!(A.dense[l] = (float *)M.get(P.dense_bytes[l], guard == 1))) return -5; }
        for (int k = 0; k < 3; ++k) { if (!(A.patch[k] = (float *)M.get(sizeof(float) * 2 * (size_t)n_pairs * gfw_dis_patches(P.lw[finest], P.lh[finest]), guard == 1))) return -5; }
        for (int k = 0; k < GFW_VARREF_PLANES && VP.launches; ++k) { if (!(plane[k] = (float *)M.get(VP.plane_bytes, guard == 1))) return -5; }
    }
    std::vector<float> gp((size_t)P.grid.nodes * n_frames * 2 + 1);
    std::vector<int32_t> gc((size_t)n_frames + 1);
    G.grid_points = grid_points ? grid_points : gp.data(); G.grid_counts = grid_counts ? grid_counts : gc.data();
    A.grid_points = G.grid_points; A.grid_counts = G.grid_counts;
    if (flow) A.dense[finest] = flow;
    A.out_pair_first = out_pair_first; A.points_a = points_a; A.points_b = points_b;
    int rc = 0;
    for (int l = 1; l <= P.coarsest && !rc; ++l) {
        emu_dsrc = A.lv[l - 1]; emu_ddst = (uint8_t *)A.lv[l].base; emu_ddw = P.lw[l]; emu_ddh = P.lh[l];
        emu_dblocks = (unsigned)(((size_t)emu_ddw * emu_ddh + 255) / 256);
        rc = emu_varref_run((int)emu_dblocks * n_frames, emu_dis_pyramid_body);
    }
    if (!rc) rc = emu_varref_run(n_frames, emu_dis_grid_body);
    for (int l = P.coarsest; l >= finest && !rc; --l) {
        emu_dlevel = l;
        for (emu_dpass = 0; emu_dpass < 3 && !rc; ++emu_dpass) {
            emu_dblocks = (unsigned)gfw_dis_patches(P.lw[l], P.lh[l]);
            rc = emu_varref_run((int)emu_dblocks * n_pairs, emu_dis_pass_body);
        }
        const unsigned full = (unsigned)(((size_t)P.lw[l] * P.lh[l] + 255) / 256), half = (unsigned)(((size_t)((P.lw[l] + 1) / 2) * P.lh[l] + 255) / 256);
        emu_dblocks = full;
        if (!rc) rc = emu_varref_run((int)full * n_pairs, emu_dis_dense_body);
        if (!VP.launches) continue;
        emu_vR = gfw_varref_level(VP, V, A, l, (char *)vwork.data());
        if (guard) for (int k = 0; k < GFW_VARREF_PLANES; ++k) {                 // the level's planes end (or start) where the level's pixels do
            const size_t used = sizeof(float) * (size_t)n_pairs * P.lw[l] * P.lh[l];
            emu_vR.plane[k] = guard == 1 ? (float *)((char *)plane[k] + (VP.plane_bytes - used)) : plane[k];
        }
        if (!rc) rc = emu_varref_run((int)full * n_pairs, emu_varref_prepare_body);
        for (int fp = 0; fp < V.fixed_point_iters && !rc; ++fp) {
            rc = emu_varref_run((int)full * n_pairs, emu_varref_coeff_body);
            for (int it = 0; it < V.sor_iters && !rc; ++it)
                for (emu_vcolour = 0; emu_vcolour < 2 && !rc; ++emu_vcolour) { emu_dblocks = half; rc = emu_varref_run((int)half * n_pairs, emu_varref_sor_body); emu_dblocks = full; }
        }
        if (!rc) rc = emu_varref_run((int)full * n_pairs, emu_varref_apply_body);
    }
    if (!rc) rc = emu_varref_run(1, emu_dis_scan_body);
    if (!rc) rc = emu_varref_run(n_pairs, emu_dis_nodes_body);
    if (launches) *launches = emu_vlaunches;
    return rc;
}
