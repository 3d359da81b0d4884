// emu_sync_gyro_driver.inc — TEST INFRASTRUCTURE: launches of the gyro-match search's kernels (gfw_sync_gyro.hip, compiled for the host above) on the fibers, in the order
// gfw_sync_gyro_costs / gfw_sync_gyro_search enqueue them, over what gfw_gyro_stage (the entry points' own host staging, gfw_sync_gyro_host.h) makes of the caller's arrays.
// The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: the pick stage is launched that way on the device too; a cost workgroup's (block of
// candidates, range) is unfolded from the linear index.
#include "emu_fibers.inc"
#include "../../gyroflow_amd/csrc/gfw_sync_gyro_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static GfwGyroArgs emu_gA; static GfwGyroPickArgs emu_gR; static unsigned emu_gblocks;
static void emu_gyro_cost_body() {
    const unsigned b = emu_cur->bid.x;
    emu_cur->bid = dim3{b % emu_gblocks, b / emu_gblocks, 0};
    gfw_gyro_cost_kernel(emu_gA);
}
static void emu_gyro_pick_body() { gfw_gyro_pick_kernel(emu_gR); }
static int emu_gyro_costs_launch(int n_ranges, int max_candidates) {          // gfw_launch_gyro_costs: zero-sized launches are skipped
    if (n_ranges <= 0 || max_candidates <= 0) return 0;
    emu_gblocks = (unsigned)((max_candidates + GFW_GYRO_LANES - 1) / GFW_GYRO_LANES);
    return emu::run_grid((int)emu_gblocks * n_ranges, emu_gyro_cost_body);
}

// The arguments of gfw_sync_gyro_costs (search 0) / gfw_sync_gyro_search (search 1) with host outputs.  costs: the caller's array, entry cand_first[r] + i for candidate i of
// range r (search: n_coarse per range, from 0); fine / fine_costs [n_ranges][200]; results [n_ranges].  -> 0, or the interpreter's error.
extern "C" int gfw_emu_sync_gyro(const int32_t *est_first, const double *est, const uint8_t *est_has, const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has,
                                 int n_ranges, const int32_t *cand_first, const double *candidates, int search, double initial_offset_ms, double search_size_ms,
                                 double *costs, void *results, double *fine, double *fine_costs, int *gyro_kept) {
    if (n_ranges <= 0) return 0;
    const size_t n_coarse = search ? (size_t)gfw_gyro_key(search_size_ms) * 2 : 0;
    const size_t tot_est = (size_t)(est_first[n_ranges] - est_first[0]), tot_gyro = (size_t)(gyro_first[n_ranges] - gyro_first[0]);
    const size_t tot_cand = search ? n_coarse * (size_t)n_ranges : (size_t)(cand_first[n_ranges] - cand_first[0]);
    const GfwGyroLayout L = gfw_gyro_layout(n_ranges, tot_est, tot_gyro, tot_cand);
    std::vector<uint64_t> block(L.total / 8);                                 // ONE block of exactly the layout's bytes ("device" = host memory)
    char *h = (char *)block.data();
    GfwGyroArgs &A = emu_gA;
    memset(&A, 0, sizeof(A));
    const GfwGyroSeries se = {est_first, est, est_has}, sg = {gyro_first, gyro, gyro_has};
    const int max_cand = gfw_gyro_fill(L, se, sg, n_ranges, search ? nullptr : cand_first, candidates, n_coarse, initial_offset_ms, search_size_ms, h, h, A);
    if (gyro_kept) for (int r = 0; r < n_ranges; ++r) gyro_kept[r] = A.ranges[r].gyro_n;
    A.costs = search ? costs : costs + cand_first[0]; A.stage = 0;          // as the entry point: the caller's entries cand_first[0] ..
    int rc = emu_gyro_costs_launch(n_ranges, max_cand);
    if (rc || !search) return rc;
    GfwGyroPickArgs &R = emu_gR;
    memset(&R, 0, sizeof(R));
    R.ranges = A.ranges; R.candidates = A.candidates; R.costs = A.costs; R.results = (gfw_sync_result *)results; R.fine = fine; R.stage = 0;
    rc = emu::run_grid(n_ranges, emu_gyro_pick_body);
    if (rc) return rc;
    A.candidates = fine; A.costs = fine_costs; A.gate = R.results; A.stage = 1;
    rc = emu_gyro_costs_launch(n_ranges, GFW_GYRO_FINE);
    if (rc) return rc;
    R.candidates = fine; R.costs = fine_costs; R.fine_costs = fine_costs; R.stage = 1;
    return emu::run_grid(n_ranges, emu_gyro_pick_body);
}
