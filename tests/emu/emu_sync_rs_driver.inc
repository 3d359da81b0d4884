// emu_sync_rs_driver.inc — TEST INFRASTRUCTURE: launches of the rs-sync search's kernels (gfw_sync_rs.hip, compiled for the host above) on the fibers, in the order
// gfw_sync_rs_costs / gfw_sync_rs_search enqueue them, over what gfw_rs_check / gfw_rs_layout / gfw_rs_fill / gfw_rs_constants / gfw_rs_round (the entry points' own
// host code, gfw_sync_rs_host.h) make of the caller's arrays.  The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: the prepare and pick stages
// are launched that way on the device too; a cost workgroup is one wave — the lanes beyond do not exist on the device and leave at once — and its (candidate, pair)
// is unfolded from the linear index.  The dynamic LDS of the cost stage is a static array of the largest size and the wave's butterfly a rendezvous of its lanes
// (GFW_RS_DYN_LDS, __shfl_xor: defined in front of the source by tests/_emu_rs_sync.py).  Every array of the work space is a mapping of its own between two
// inaccessible pages, its last byte (guard 1) or its first (guard 2) against one of them.
#include "emu_fibers.inc"
#include <sys/mman.h>
#include <unistd.h>
#include <utility>
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_sync_rs_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static gfw_kernel_params emu_rP; static GfwCommon emu_rC; static GfwRsArgs emu_rA; static unsigned emu_rcands;
static void emu_rs_prepare_body() {
    if (emu_rC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_rs_prepare_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_rP, emu_rC, emu_rA);
    else gfw_rs_prepare_kernel<-1>(emu_rP, emu_rC, emu_rA);
}
static void emu_rs_cost_body() { if (emu_cur->tid.y) return; const unsigned b = emu_cur->bid.x; emu_cur->bid = dim3{b % emu_rcands, b / emu_rcands, 0}; gfw_rs_cost_kernel(emu_rA); }
static void emu_rs_pick_body() { gfw_rs_pick_kernel(emu_rA); }

struct EmuRsGuarded {
    std::vector<std::pair<void *, size_t>> maps;
    ~EmuRsGuarded() { for (auto &m : maps) munmap(m.first, m.second); }
    double *get(size_t doubles, int guard) {
        const size_t bytes = doubles * 8 + 8, page = (size_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
        char *m = (char *)mmap(nullptr, body + 2 * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == (char *)MAP_FAILED) return nullptr;
        maps.push_back({m, body + 2 * page});
        if (mprotect(m, page, PROT_NONE) || mprotect(m + page + body, page, PROT_NONE)) return nullptr;
        return (double *)(m + page + (guard == 1 ? body - doubles * 8 : 0));
    }
};
static int emu_rs_costs_launch(int max_candidates) {
    if (emu_rA.n_pairs <= 0 || max_candidates <= 0) return 0;
    emu_rcands = (unsigned)max_candidates;
    return emu::run_grid(max_candidates * emu_rA.n_pairs, emu_rs_cost_body);
}

// The arguments of gfw_sync_rs_search (search 1) / gfw_sync_rs_costs (search 0) with host outputs; settings: (rounds, refine, hypotheses, refits, jacobi_sweeps),
// reals: (frame_readout_time_ms, step_s, loss_scale, initial_delay_s, radius_s).  results: [n_ranges][5] words of gfw_sync_result.  -> 0, -1 with the reason in
// `why` where the entry point's check refuses, or the interpreter's error.  round_candidates / round_costs may be NULL: the work space serves.
extern "C" int gfw_emu_sync_rs(const void *kp, const void *common, int video_w, int video_h, int flow_w, int flow_h, const int32_t *settings, const double *reals,
                               int search, const int32_t *range_first, int n_ranges, const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a,
                               const float *points_b, int n_pairs, const int64_t *track_ts_us, const double *track_wxyz, int n_track, const int32_t *cand_first,
                               const double *candidates, int n_candidates, double *costs, void *results, double *round_candidates, double *round_costs, int guard,
                               char *why, size_t why_cap) {
    memcpy(&emu_rP, kp, sizeof(emu_rP)); memcpy(&emu_rC, common, sizeof(emu_rC));
    const GfwRsInputs I = {range_first, n_ranges, pair_ts_us, pair_first, points_a, points_b, n_pairs, track_ts_us, track_wxyz, n_track,
                           search ? nullptr : cand_first, search ? nullptr : candidates, search ? 0 : n_candidates};
    GfwRsSettings S;
    memset(&S, 0, sizeof(S));
    S.rounds = settings[0]; S.refine = settings[1]; S.hypotheses = settings[2]; S.refits = settings[3]; S.sweeps = settings[4];
    S.step_s = reals[1]; S.loss_scale = reals[2]; S.initial_delay_s = reals[3]; S.radius_s = reals[4]; S.search = search != 0;
    if (!gfw_rs_check(I, S, why, why_cap)) return -1;
    if (n_ranges == 0 || (!search && n_candidates == 0)) return 0;
    const GfwRsLayout L = gfw_rs_layout(I);
    std::vector<uint64_t> block(L.total / 8 + 1);                             // ONE block of the layout's bytes ("device" = host memory)
    char *h = (char *)block.data();
    GfwRsArgs &A = emu_rA;
    memset(&A, 0, sizeof(A));
    gfw_rs_fill(L, I, h, h, A);
    gfw_rs_constants(video_w, video_h, flow_w, flow_h, reals[0], S, A);
    const int n0 = search ? gfw_rs_round0_count(S.radius_s, S.step_s) : 0;
    const size_t row = search ? (size_t)n0 + (size_t)(S.rounds - 1) * GFW_RS_LATER : 0, rows = row * (size_t)n_ranges;
    const size_t n_pc = search ? (size_t)n_pairs * (size_t)(n0 > GFW_RS_LATER ? n0 : GFW_RS_LATER) : L.pair_costs;
    EmuRsGuarded G;
    std::vector<double> prep(guard ? 1 : 8 * L.points + 1), pc(guard ? 1 : n_pc + 1), wc(guard ? 1 : rows + 1), ws(guard ? 1 : rows + 1);
    A.prep = guard ? G.get(8 * L.points, guard) : prep.data(); A.pair_costs = guard ? G.get(n_pc, guard) : pc.data();
    double *w_cand = guard ? G.get(rows, guard) : wc.data(), *w_sums = guard ? G.get(rows, guard) : ws.data();
    if (!A.prep || !A.pair_costs || !w_cand || !w_sums) return -5;
    int rc = A.total > 0 ? emu::run_grid((int)((2 * (size_t)A.total + GFW_RS_LANES - 1) / GFW_RS_LANES), emu_rs_prepare_body) : 0;
    if (search) {
        A.cand_all = round_candidates ? round_candidates : w_cand; A.sums_all = round_costs ? round_costs : w_sums;
        A.results = (gfw_sync_result *)results;
        for (int round = 0; round < S.rounds && !rc; ++round) {
            gfw_rs_round(S, round, A);
            rc = emu_rs_costs_launch(A.n_cand);
            if (!rc) rc = emu::run_grid(n_ranges, emu_rs_pick_body);
        }
    } else {
        A.mode = 0; A.sums_all = costs;
        if (!rc) rc = emu_rs_costs_launch(L.max_cand);
        if (!rc) rc = emu::run_grid(n_ranges, emu_rs_pick_body);
    }
    return rc;
}
