// emu_dis_driver.inc — TEST INFRASTRUCTURE: launches of the DIS dense flow's kernels (gfw_dis.hip, and the grid kernel of gfw_flow.hip, both compiled for the host
// above) on the fibers, in the order gfw_flow_dis enqueues them, over what gfw_dis_check / gfw_dis_plan / gfw_dis_fill (the entry point's own host code,
// gfw_dis_host.h) make of the caller's arrays.  The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: a kernel the device launches with 64
// lanes runs on the first wave's fibers (the other three return at once, as lanes that do not exist); a (block, frame) or (patch, pair) workgroup is unfolded from
// the linear index.  Every pyramid level, dense field and patch-value array is a mapping of its own between two inaccessible pages, its last byte (guard 1) or its
// first (guard 2) against one of them; so are the outputs where the caller places them so.
#include "emu_fibers.inc"
#include <sys/mman.h>
#include <unistd.h>
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_flow_host.h"
#include "../../gyroflow_amd/csrc/gfw_dis_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static GfwDisArgs emu_dA; static GfwFlowArgs emu_dG; static GfwDisLevel emu_dsrc; static uint8_t *emu_ddst; static int emu_ddw, emu_ddh, emu_dlevel, emu_dpass; static unsigned emu_dblocks;
static void emu_dis_unfold() { const unsigned b = emu_cur->bid.x; emu_cur->bid = dim3{b % emu_dblocks, b / emu_dblocks, 0}; }
static void emu_dis_pyramid_body() { emu_dis_unfold(); gfw_dis_pyramid_kernel(emu_dsrc, emu_ddst, emu_ddw, emu_ddh); }
static void emu_dis_grid_body() { if (emu_cur->tid.y) return; gfw_flow_grid_kernel(emu_dG); }
static void emu_dis_pass_body() { if (emu_cur->tid.y) return; emu_dis_unfold(); gfw_dis_pass_kernel(emu_dA, emu_dlevel, emu_dpass); }
static void emu_dis_dense_body() { emu_dis_unfold(); gfw_dis_dense_kernel(emu_dA, emu_dlevel); }
static void emu_dis_scan_body() { gfw_dis_scan_kernel(emu_dA); }
static void emu_dis_nodes_body() { if (emu_cur->tid.y) return; gfw_dis_nodes_kernel(emu_dA); }

struct EmuDisGuarded {
    std::vector<std::pair<void *, size_t>> maps;
    ~EmuDisGuarded() { for (auto &m : maps) munmap(m.first, m.second); }
    uint8_t *get(size_t bytes, bool at_end) {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
        char *m = (char *)mmap(nullptr, body + 2 * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == (char *)MAP_FAILED) return nullptr;
        maps.push_back({m, body + 2 * page});
        if (mprotect(m, page, PROT_NONE) || mprotect(m + page + body, page, PROT_NONE)) return nullptr;
        return (uint8_t *)(m + page + (at_end ? body - bytes : 0));
    }
};

// The arguments of gfw_flow_dis with host frames and host outputs (points_a / points_b: room for every node of every pair).  -> 0, -1 with the reason in `why` where
// the entry point's check refuses, or the interpreter's error.  grid_points / grid_counts / flow may be NULL: work space serves, as in the entry point.
extern "C" int gfw_emu_dis(int width, int height, int stride, int finest, int variational_iters, int reserved, const void *frames, int n_frames, const int32_t *pair_frames,
                           int n_pairs, float *grid_points, int32_t *grid_counts, float *flow, int32_t *out_pair_first, float *points_a, float *points_b, int guard,
                           char *why, size_t why_cap) {
    const GfwDisInputs I = {width, height, stride, finest, variational_iters, reserved, frames, 1, n_frames, pair_frames, n_pairs};      // "device" = host memory: the frames are used in place
    if (!gfw_dis_check(I, why, why_cap)) return -1;
    if (n_pairs == 0) return 0;
    if (!out_pair_first || !points_a || !points_b) { snprintf(why, why_cap, "bad DIS flow arguments (a null out_pair_first / points_a / points_b array)"); return -1; }
    const GfwDisPlan P = gfw_dis_plan(I);
    std::vector<uint64_t> block(P.total / 8 + 1), work(guard ? 1 : P.work_bytes / 8 + 1);
    char *h = (char *)block.data();
    GfwDisArgs &A = emu_dA; GfwFlowArgs &G = emu_dG;
    memset(&A, 0, sizeof(A)); memset(&G, 0, sizeof(G));
    gfw_dis_fill(P, I, h, h, (char *)work.data(), A, G);
    EmuDisGuarded M;
    if (guard) {                                                            // every array of the work space a mapping of its own
        for (int l = 1; l <= P.coarsest; ++l) { if (!(A.lv[l].base = M.get((size_t)n_frames * P.lw[l] * P.lh[l], guard == 1))) return -5; }
        for (int l = finest; l <= P.coarsest; ++l) { if (!(A.dense[l] = (float *)M.get(P.dense_bytes[l], guard == 1))) return -5; }
        for (int k = 0; k < 3; ++k) { if (!(A.patch[k] = (float *)M.get(sizeof(float) * 2 * (size_t)n_pairs * gfw_dis_patches(P.lw[finest], P.lh[finest]), guard == 1))) return -5; }
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
        rc = emu::run_grid((int)emu_dblocks * n_frames, emu_dis_pyramid_body);
    }
    if (!rc) rc = emu::run_grid(n_frames, emu_dis_grid_body);
    for (int l = P.coarsest; l >= finest && !rc; --l) {
        emu_dlevel = l;
        for (emu_dpass = 0; emu_dpass < 3 && !rc; ++emu_dpass) {
            emu_dblocks = (unsigned)gfw_dis_patches(P.lw[l], P.lh[l]);
            rc = emu::run_grid((int)emu_dblocks * n_pairs, emu_dis_pass_body);
        }
        if (!rc) {
            emu_dblocks = (unsigned)(((size_t)P.lw[l] * P.lh[l] + 255) / 256);
            rc = emu::run_grid((int)emu_dblocks * n_pairs, emu_dis_dense_body);
        }
    }
    if (!rc) rc = emu::run_grid(1, emu_dis_scan_body);
    if (!rc) rc = emu::run_grid(n_pairs, emu_dis_nodes_body);
    return rc;
}
