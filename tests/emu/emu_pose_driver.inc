// emu_pose_driver.inc — TEST INFRASTRUCTURE: launches of the pose estimation's kernels (gfw_pose.hip, compiled for the host above) on the fibers, in the order
// gfw_pose_almeida enqueues them, over what gfw_pose_check / gfw_pose_fill / gfw_pose_constants (the entry point's own host code, gfw_pose_host.h) make of the
// caller's arrays.  The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: the prepare and pick stages are launched that way on the device too;
// a fit or count workgroup's (block of rounds, pair) is unfolded from the linear index.
#include "emu_fibers.inc"
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_pose_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static gfw_kernel_params emu_pP; static GfwCommon emu_pC; static GfwPoseArgs emu_pA; static unsigned emu_pblocks;
static void emu_pose_prepare_body() {
    if (emu_pC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_pose_prepare_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_pP, emu_pC, emu_pA);
    else gfw_pose_prepare_kernel<-1>(emu_pP, emu_pC, emu_pA);
}
static void emu_pose_unfold() { const unsigned b = emu_cur->bid.x; emu_cur->bid = dim3{b % emu_pblocks, b / emu_pblocks, 0}; }
static void emu_pose_fit_body() { emu_pose_unfold(); gfw_pose_fit_kernel(emu_pA); }
static void emu_pose_count_body() { emu_pose_unfold(); gfw_pose_count_kernel(emu_pA); }
static void emu_pose_pick_body() { gfw_pose_pick_kernel(emu_pA); }

// The arguments of gfw_pose_almeida with host outputs (cfg: gfw_pose_almeida_cfg's fields).  -> 0, -1 with the reason in `why` where the entry point's check refuses,
// or the interpreter's error.  round_inliers / round_fits may be NULL: the work space serves, as in the entry point.
extern "C" int gfw_emu_pose(const void *kp, const void *common, int video_w, int video_h, int flow_w, int flow_h, int num_iters, int num_samples, float inlier_angle_deg,
                            const double *K, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs, const int32_t *triples,
                            const int32_t *sample_first, const int32_t *samples, float *quats, double *rotations, int32_t *best, int32_t *round_inliers, float *round_fits,
                            char *why, size_t why_cap) {
    memcpy(&emu_pP, kp, sizeof(emu_pP)); memcpy(&emu_pC, common, sizeof(emu_pC));
    const GfwPoseInputs I = {pair_first, points_a, points_b, n_pairs, triples, sample_first, samples, num_iters, num_samples};
    if (!gfw_pose_check(I, why, why_cap)) return -1;
    if (n_pairs == 0) return 0;
    const GfwPoseLayout S = gfw_pose_layout(I);
    std::vector<uint64_t> block(S.total / 8 + 1);                             // ONE block of the layout's bytes ("device" = host memory)
    char *h = (char *)block.data();
    GfwPoseArgs &A = emu_pA;
    memset(&A, 0, sizeof(A));
    gfw_pose_fill(S, I, h, h, A);
    gfw_pose_constants(video_w, video_h, flow_w, flow_h, inlier_angle_deg, K, A);
    const size_t rounds = (size_t)n_pairs * (size_t)num_iters, total = (size_t)A.total;
    std::vector<float4> pm(total + 1), rays(total + 1);
    std::vector<float2> derivs(3 * total + 1);
    std::vector<float> fits(4 * rounds + 1);
    std::vector<int32_t> counts(rounds + 1);
    A.pm = pm.data(); A.rays = rays.data(); A.derivs = derivs.data();
    A.fits = round_fits ? round_fits : fits.data(); A.counts = round_inliers ? round_inliers : counts.data();
    A.quats = quats; A.rotations = rotations; A.best = best;
    int rc = A.total > 0 ? emu::run_grid((A.total + GFW_POSE_LANES - 1) / GFW_POSE_LANES, emu_pose_prepare_body) : 0;
    if (!rc && num_iters > 0) { emu_pblocks = (unsigned)((num_iters + GFW_POSE_LANES - 1) / GFW_POSE_LANES); rc = emu::run_grid((int)emu_pblocks * n_pairs, emu_pose_fit_body); }
    if (!rc && num_iters > 0) { emu_pblocks = (unsigned)((num_iters + 3) / 4); rc = emu::run_grid((int)emu_pblocks * n_pairs, emu_pose_count_body); }
    if (!rc) rc = emu::run_grid(n_pairs, emu_pose_pick_body);
    return rc;
}
