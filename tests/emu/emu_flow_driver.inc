// emu_flow_driver.inc — TEST INFRASTRUCTURE: launches of the optical flow's kernels (gfw_flow.hip, compiled for the host above) on the fibers, in the order
// gfw_flow_pyrlk enqueues them, over what gfw_flow_check / gfw_flow_plan / gfw_flow_fill (the entry point's own host code, gfw_flow_host.h) make of the caller's
// arrays.  The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: a kernel the device launches with 64 lanes runs on the first wave's fibers
// (the other three return at once, as lanes that do not exist); a (block, frame) or (feature, pair) workgroup is unfolded from the linear index.
// Every pyramid level is a mapping of its own between two inaccessible pages, its last byte (guard 1) or its first (guard 2) against one of them.
#include "emu_fibers.inc"
#include <sys/mman.h>
#include <unistd.h>
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_flow_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static GfwFlowArgs emu_fA; static GfwFlowLevel emu_fsrc; static uint8_t *emu_fdst; static int emu_fdw, emu_fdh; static unsigned emu_fblocks;
static void emu_flow_unfold() { const unsigned b = emu_cur->bid.x; emu_cur->bid = dim3{b % emu_fblocks, b / emu_fblocks, 0}; }
static void emu_flow_pyramid_body() { emu_flow_unfold(); gfw_flow_pyramid_kernel(emu_fsrc, emu_fdst, emu_fdw, emu_fdh); }
static void emu_flow_grid_body() { if (emu_cur->tid.y) return; gfw_flow_grid_kernel(emu_fA); }
static void emu_flow_track_body() { if (emu_cur->tid.y) return; emu_flow_unfold(); gfw_flow_track_kernel(emu_fA); }
static void emu_flow_scan_body() { gfw_flow_scan_kernel(emu_fA); }
static void emu_flow_compact_body() { if (emu_cur->tid.y) return; gfw_flow_compact_kernel(emu_fA); }

struct EmuGuarded {
    std::vector<std::pair<void *, size_t>> maps;
    ~EmuGuarded() { for (auto &m : maps) munmap(m.first, m.second); }
    uint8_t *get(size_t bytes, bool at_end) {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
        char *m = (char *)mmap(nullptr, body + 2 * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == (char *)MAP_FAILED) return nullptr;
        maps.push_back({m, body + 2 * page});
        if (mprotect(m, page, PROT_NONE) || mprotect(m + page + body, page, PROT_NONE)) return nullptr;
        return (uint8_t *)(m + page + (at_end ? body - bytes : 0));
    }
};

// The arguments of gfw_flow_pyrlk with host frames and host outputs (points_a / points_b: room for every raw slot).  -> 0, -1 with the reason in `why` where the
// entry point's check refuses, or the interpreter's error.  iters / grid_points / grid_counts may be NULL: work space serves, as in the entry point.
extern "C" int gfw_emu_flow(int width, int height, int stride, int mode, int reserved, const void *frames, int n_frames, const int32_t *pair_frames, int n_pairs,
                            const int32_t *feat_first, const float *features, float *next, uint8_t *status, int32_t *iters, float *grid_points, int32_t *grid_counts,
                            int32_t *out_pair_first, float *points_a, float *points_b, int guard, char *why, size_t why_cap) {
    const GfwFlowInputs I = {width, height, stride, mode, reserved, frames, 1, n_frames, pair_frames, n_pairs, feat_first, features};      // "device" = host memory: the frames are used in place
    if (!gfw_flow_check(I, why, why_cap)) return -1;
    if (n_pairs == 0) return 0;
    const GfwFlowPlan P = gfw_flow_plan(I);
    std::vector<uint64_t> block(P.total / 8 + 1), work(P.pyramid_bytes / 8 + 1);
    char *h = (char *)block.data();
    GfwFlowArgs &A = emu_fA;
    memset(&A, 0, sizeof(A));
    gfw_flow_fill(P, I, h, h, (const uint8_t *)work.data(), A);
    EmuGuarded G;
    uint8_t *level[GFW_FLOW_LEVELS] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 1; l <= P.top; ++l) {
        level[l] = guard ? G.get((size_t)n_frames * P.lw[l] * P.lh[l], guard == 1) : (uint8_t *)work.data() + P.level_at[l];
        if (!level[l]) return -5;
        A.lv[l].base = level[l];
    }
    std::vector<float> gp((size_t)P.grid.nodes * n_frames * 2 + 1);
    std::vector<int32_t> gc((size_t)n_frames + 1);
    A.next = next; A.status = status; A.iters = iters;
    if (mode == GFW_FLOW_MODE_GRID) { A.grid_points = grid_points ? grid_points : gp.data(); A.grid_counts = grid_counts ? grid_counts : gc.data(); }
    A.out_pair_first = out_pair_first; A.points_a = points_a; A.points_b = points_b;
    int rc = 0;
    for (int l = 1; l <= P.top && !rc; ++l) {
        emu_fsrc = A.lv[l - 1]; emu_fdst = level[l]; emu_fdw = P.lw[l]; emu_fdh = P.lh[l];
        emu_fblocks = (unsigned)(((size_t)emu_fdw * emu_fdh + 255) / 256);
        rc = emu::run_grid((int)emu_fblocks * n_frames, emu_flow_pyramid_body);
    }
    if (!rc && mode == GFW_FLOW_MODE_GRID) rc = emu::run_grid(n_frames, emu_flow_grid_body);
    if (!rc && A.max_features > 0) { emu_fblocks = (unsigned)A.max_features; rc = emu::run_grid(A.max_features * n_pairs, emu_flow_track_body); }
    if (!rc) rc = emu::run_grid(1, emu_flow_scan_body);
    if (!rc) rc = emu::run_grid(n_pairs, emu_flow_compact_body);
    return rc;
}
