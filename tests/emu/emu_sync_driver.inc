// emu_sync_driver.inc — TEST INFRASTRUCTURE: launches of the sync search's kernels (gfw_sync.hip, compiled for the host above) on the fibers, in the order
// gfw_sync_visual_costs / gfw_sync_visual_search enqueue them.  The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: the lens and reduce stages
// are launched that way on the device too; a cost workgroup is one wave (the lanes beyond leave at once) and its (candidate, pair) is unfolded from the linear index.
#include "emu_fibers.inc"
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_sync_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static gfw_kernel_params emu_sP; static GfwCommon emu_sC; static GfwSyncArgs emu_sA; static GfwSyncReduceArgs emu_sR;
static void emu_sync_rays_body() {
    if (emu_sC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_sync_rays_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_sP, emu_sC, emu_sA);
    else gfw_sync_rays_kernel<-1>(emu_sP, emu_sC, emu_sA);
}
static void emu_sync_cost_body() {
    if (emu_cur->tid.y >= 1) return;
    const unsigned b = emu_cur->bid.x;
    emu_cur->bid = dim3{b / (unsigned)emu_sA.n_pairs, b % (unsigned)emu_sA.n_pairs, 0};
    gfw_sync_cost_kernel(emu_sA);
}
static void emu_sync_reduce_body() { gfw_sync_reduce_kernel(emu_sR); }
static int emu_sync_costs_launch(int n) {                                     // gfw_launch_sync_costs: zero-sized launches are skipped
    if (n <= 0 || emu_sA.n_pairs <= 0) return 0;
    return emu::run_grid(n * emu_sA.n_pairs, emu_sync_cost_body);
}

// The arguments of gfw_sync_visual_costs (mode < 0: the costs of the `n` caller-given `candidates`, result NULL) / gfw_sync_visual_search (mode 0 / 1: `n` is the count
// of coarse candidates the caller sized `costs` for — made here by the entry point's own rule, which has to agree).  What the entry stages goes into ONE block of
// exactly the layout's bytes ("device" = host memory).  work: rays [2 * total][4] f32, partial [max(n, 200) * max(n_pairs, 1)] u64, fine [200][2] f64 — the caller's,
// as the context's device work space.
extern "C" int gfw_emu_sync(const void *kp, const void *common, const int64_t *org_ts, const double *org_q, int org_n, const int64_t *sm_ts, const double *sm_q, int sm_n,
                            const int64_t *off_ts, const double *off_ms, int off_n, double duration_ms, const gfw_sync_search *search,
                            const int64_t *pair_ts, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs, const double *candidates, int n, int mode,
                            double initial_offset_ms, double search_size_ms, double frame_readout_time_ms, double scaled_fps,
                            float *rays, unsigned long long *partial, double *fine, double *costs, float *mapped, void *result, double *fine_costs) {
    memcpy(&emu_sP, kp, sizeof(emu_sP)); memcpy(&emu_sC, common, sizeof(emu_sC));
    if (mode >= 0 && n != (int)gfw_sync_coarse_steps(mode, search_size_ms, scaled_fps) * (mode ? 2 : 1)) return -2;
    GfwSyncArgs &A = emu_sA;
    memset(&A, 0, sizeof(A));
    const GfwSyncLayout S = gfw_sync_layout(n_pairs, n_pairs ? pair_first[n_pairs] : 0, (size_t)n);
    static std::vector<uint64_t> block;
    block.assign(S.total / 8, 0);
    char *h = (char *)block.data();
    gfw_sync_fill(S, pair_ts, pair_first, points_a, points_b, n_pairs, mode < 0 ? candidates : nullptr, n, mode, initial_offset_ms, search_size_ms, frame_readout_time_ms, h, h, A);
    A.T = GfwTracks{org_ts, org_q, org_n, sm_ts, sm_q, sm_n, off_ts, off_ms, off_n, duration_ms};
    for (int i = 0; i < 9; ++i) A.F.new_k[i] = search->new_k[i];
    A.F.video_rotation_deg = search->video_rotation_deg;
    A.rays = (float4 *)rays; A.partial = partial; A.mapped = mapped;
    A.w = (float)search->width; A.h = (float)search->height;
    A.horizontal = search->horizontal_readout; A.readout_dim = search->horizontal_readout ? search->width : search->height;
    GfwSyncReduceArgs &R = emu_sR;
    memset(&R, 0, sizeof(R));
    R.partial = partial; R.candidates = A.candidates; R.costs = costs; R.result = (gfw_sync_result *)result; R.fine = fine;
    R.n = n; R.n_pairs = A.n_pairs; R.column = mode == 1 ? 1 : 0; R.stage = 0;
    int rc = A.total > 0 ? emu::run_grid((A.total * 2 + 255) / 256, emu_sync_rays_body) : 0;
    if (!rc) rc = emu_sync_costs_launch(n);
    if (!rc) rc = emu::run_grid(1, emu_sync_reduce_body);
    if (rc || mode < 0) return rc;
    A.candidates = fine; A.gate = R.result; A.mapped = nullptr;
    rc = emu_sync_costs_launch(GFW_SYNC_FINE);
    R.candidates = fine; R.costs = fine_costs; R.n = GFW_SYNC_FINE; R.stage = 1;
    if (!rc) rc = emu::run_grid(1, emu_sync_reduce_body);
    return rc;
}

// Test-only entry: the fold and the reduce stage of the kernel source over TABULATED mapped points — mapped [n][total][2][2] as gfw_sync_visual_costs writes them —
// so that constructed point sets drive the selection through its edge cases.  stage 0 also fills `result` and the fine candidates.
struct EmuSyncTable {
    const float *mapped; size_t cand; int total, first;
    float4 operator()(int i) const { const float *m = mapped + (cand * (size_t)total + first + i) * 4; return float4{m[0], m[1], m[2], m[3]}; }
};
static const float *emu_tmapped; static const int32_t *emu_tfirst; static int emu_tpairs, emu_ttotal; static float emu_tw, emu_th; static unsigned long long *emu_tpartial;
static uint32_t emu_tdist[GFW_SYNC_PAIR_MAX]; static unsigned long long emu_tsum;
static void emu_sync_table_body() {
    if (emu_cur->tid.y >= 1) return;
    const unsigned cand = emu_cur->bid.x / (unsigned)emu_tpairs, pair = emu_cur->bid.x % (unsigned)emu_tpairs;
    const int t = threadIdx.x;
    const EmuSyncTable map{emu_tmapped, cand, emu_ttotal, emu_tfirst[pair]};
    const unsigned long long total = gfw_sync_fold(map, t, emu_tfirst[pair + 1] - emu_tfirst[pair], emu_tw, emu_th, emu_tdist, &emu_tsum);
    if (t == 0) emu_tpartial[(size_t)cand * emu_tpairs + pair] = total;
}
extern "C" int gfw_emu_sync_table(const float *mapped, const int32_t *pair_first, int n_pairs, int total, int width, int height, const double *candidates, int n, int column,
                                  unsigned long long *partial, double *fine, double *costs, void *result) {
    emu_tmapped = mapped; emu_tfirst = pair_first; emu_tpairs = n_pairs; emu_ttotal = total; emu_tw = (float)width; emu_th = (float)height; emu_tpartial = partial;
    int rc = n > 0 && n_pairs > 0 ? emu::run_grid(n * n_pairs, emu_sync_table_body) : 0;
    GfwSyncReduceArgs &R = emu_sR;
    memset(&R, 0, sizeof(R));
    R.partial = partial; R.candidates = candidates; R.costs = costs; R.result = (gfw_sync_result *)result; R.fine = fine;
    R.n = n; R.n_pairs = n_pairs; R.column = column; R.stage = 0;
    if (!rc) rc = emu::run_grid(1, emu_sync_reduce_body);
    return rc;
}

// Test-only entry: gfw_point_map (no shifts, no mesh, lens_correction_amount 1.0) beside its two halves composed, point by point -> [n][2] f32 each
extern "C" void gfw_emu_sync_point_split(const void *kp, const void *common, const float *points, const float *rotations, int n, float *whole, float *halves) {
    memcpy(&emu_sP, kp, sizeof(emu_sP)); memcpy(&emu_sC, common, sizeof(emu_sC));
    for (int i = 0; i < n; ++i) {
        const float x = points[i * 2], y = points[i * 2 + 1], *rot = rotations + (size_t)i * 9;
        float2 a, b = float2{-1000000.0f, -1000000.0f};
        float ptx = 0.0f, pty = 0.0f;
        if (emu_sC.model == GFW_MODEL_OPENCV_FISHEYE) {
            a = gfw_point_map<GFW_MODEL_OPENCV_FISHEYE>(emu_sP, emu_sC, x, y, rot, nullptr, nullptr, 0, 1.0f, 1.0f);
            if (gfw_point_ray<GFW_MODEL_OPENCV_FISHEYE>(emu_sP, emu_sC, x, y, ptx, pty)) b = gfw_point_project(ptx, pty, rot);
        } else {
            a = gfw_point_map<-1>(emu_sP, emu_sC, x, y, rot, nullptr, nullptr, 0, 1.0f, 1.0f);
            if (gfw_point_ray<-1>(emu_sP, emu_sC, x, y, ptx, pty)) b = gfw_point_project(ptx, pty, rot);
        }
        whole[i * 2] = a.x; whole[i * 2 + 1] = a.y; halves[i * 2] = b.x; halves[i * 2 + 1] = b.y;
    }
}
