// emu_pose_essential_driver.inc — TEST INFRASTRUCTURE: launches of the essential-matrix pose estimation's kernels (gfw_pose_essential.hip, compiled for the host
// above) on the fibers, in the order gfw_pose_essential enqueues them, over what gfw_pose_ess_check / gfw_pose_ess_fill / gfw_pose_ess_constants (the entry point's own
// host code, gfw_pose_essential_host.h) make of the caller's arrays.  The fibers interpret workgroups of 64 x 4 lanes on a one-dimensional grid: the prepare and pick stages are
// launched that way on the device too; a fit or count workgroup's (block of rounds, pair) is unfolded from the linear index.
#include "emu_fibers.inc"
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_pose_essential_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static gfw_kernel_params emu_eP; static GfwCommon emu_eC; static GfwPoseEssArgs emu_eA; static unsigned emu_eblocks;
static void emu_pe_prepare_body() {
    if (emu_eC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_pe_prepare_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_eP, emu_eC, emu_eA);
    else gfw_pe_prepare_kernel<-1>(emu_eP, emu_eC, emu_eA);
}
static void emu_pe_unfold() { const unsigned b = emu_cur->bid.x; emu_cur->bid = dim3{b % emu_eblocks, b / emu_eblocks, 0}; }
static void emu_pe_fit_body() { emu_pe_unfold(); gfw_pe_fit_kernel(emu_eA); }
static void emu_pe_count_body() { emu_pe_unfold(); gfw_pe_count_kernel(emu_eA); }
static void emu_pe_pick_body() { gfw_pe_pick_kernel(emu_eA); }

// The arguments of gfw_pose_essential with host outputs (cfg: gfw_pose_essential_cfg's fields).  -> 0, -1 with the reason in `why` where the entry point's check
// refuses, or the interpreter's error.  round_inliers / round_fits may be NULL: the work space serves, as in the entry point.
extern "C" int gfw_emu_pose_essential(const void *kp, const void *common, int video_w, int video_h, int flow_w, int flow_h, int num_iters, double inlier_threshold,
                                      int min_front, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs, const int32_t *octets,
                                      float *quats, double *rotations, double *essential, int32_t *best, int32_t *round_inliers, double *round_fits,
                                      char *why, size_t why_cap) {
    memcpy(&emu_eP, kp, sizeof(emu_eP)); memcpy(&emu_eC, common, sizeof(emu_eC));
    const GfwPoseEssInputs I = {pair_first, points_a, points_b, n_pairs, octets, num_iters};
    if (!gfw_pose_ess_check(I, why, why_cap)) return -1;
    if (n_pairs == 0) return 0;
    const GfwPoseEssLayout S = gfw_pose_ess_layout(I);
    std::vector<uint64_t> block(S.total / 8 + 1);                             // ONE block of the layout's bytes ("device" = host memory)
    char *h = (char *)block.data();
    GfwPoseEssArgs &A = emu_eA;
    memset(&A, 0, sizeof(A));
    gfw_pose_ess_fill(S, I, h, h, A);
    gfw_pose_ess_constants(video_w, video_h, flow_w, flow_h, inlier_threshold, min_front, A);
    const size_t rounds = (size_t)n_pairs * (size_t)num_iters, total = (size_t)A.total;
    std::vector<float4> und(total + 1);
    std::vector<double> fits(9 * rounds + 1);
    std::vector<int32_t> counts(rounds + 1);
    A.und = und.data();
    A.fits = round_fits ? round_fits : fits.data(); A.counts = round_inliers ? round_inliers : counts.data();
    A.quats = quats; A.rotations = rotations; A.essential = essential; A.best = best;
    int rc = A.total > 0 ? emu::run_grid((A.total + GFW_PE_LANES - 1) / GFW_PE_LANES, emu_pe_prepare_body) : 0;
    if (!rc && num_iters > 0) { emu_eblocks = (unsigned)((num_iters + GFW_PE_LANES - 1) / GFW_PE_LANES); rc = emu::run_grid((int)emu_eblocks * n_pairs, emu_pe_fit_body); }
    if (!rc && num_iters > 0) { emu_eblocks = (unsigned)((num_iters + 3) / 4); rc = emu::run_grid((int)emu_eblocks * n_pairs, emu_pe_count_body); }
    if (!rc) rc = emu::run_grid(n_pairs, emu_pe_pick_body);
    return rc;
}
