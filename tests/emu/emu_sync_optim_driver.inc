// emu_sync_optim_driver.inc — TEST INFRASTRUCTURE: launches of the sync-point choice's kernels (gfw_sync_optim.hip, compiled for the host above) on the fibers, in the order
// gfw_sync_optim_rank / gfw_sync_optim_points enqueue them, over what gfw_optim_shape / gfw_optim_fill (the entry points' own host arithmetic and staging,
// gfw_sync_optim_host.h) make of the caller's arguments.  Every kernel is launched on a one-dimensional grid of 64 x 4 lanes on the device too.  The dynamic LDS of
// the spectrum stage is a static array of the largest size here (GFW_OPTIM_DYN_LDS, defined in front of the source by tests/_emu_sync_optim.py).
#include "emu_fibers.inc"
#include <vector>
#include "../../gyroflow_amd/csrc/gfw_sync_optim_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static GfwOptimArgs emu_oA;
static void emu_optim_spectrum_body() { gfw_optim_spectrum_kernel(emu_oA); }
static void emu_optim_max_body() { gfw_optim_max_kernel(emu_oA); }
static void emu_optim_rank_body() { gfw_optim_rank_kernel(emu_oA); }
static void emu_optim_nms_body() { gfw_optim_nms_kernel(emu_oA); }
static void emu_optim_pick_body() { gfw_optim_pick_kernel(emu_oA); }
static void emu_optim_gather_body() { gfw_optim_gather_kernel(emu_oA); }

// The arguments of gfw_sync_optim_points (points 1) / gfw_sync_optim_rank (points 0) with host outputs, every output given: lf, mf, hf, rank, masked, rank_nms
// [n_windows] f32, points_ms [target] f64, n_points, shape[8] = (fft_size, n_windows, nms_radius, segment_size, bin[4]).  -> 0, or the interpreter's error.
extern "C" int gfw_emu_sync_optim(const double *gyro, long long n_samples, double sample_rate, int points, int target, const double *trim, int n_trim,
                                  float *lf, float *mf, float *hf, float *rank, float *masked, float *rank_nms, double *points_ms, int32_t *n_points, int32_t *shape) {
    if (!points) { target = 0; n_trim = 0; }
    const GfwOptimShape P = gfw_optim_shape(n_samples, sample_rate, target);
    if (P.fft_size < GFW_OPTIM_FFT_MIN || P.fft_size > GFW_OPTIM_FFT_MAX) return -10;
    shape[0] = P.fft_size; shape[1] = P.n_windows; shape[2] = P.nms_radius; shape[3] = P.segment_size;
    for (int i = 0; i < 4; ++i) shape[4 + i] = P.bin[i];
    const GfwOptimLayout L = gfw_optim_layout((size_t)n_samples, P.fft_size, n_trim);
    std::vector<uint64_t> block(L.total / 8 + 1);                             // ONE block of the layout's bytes ("device" = host memory)
    char *h = (char *)block.data();
    gfw_optim_fill(L, gyro, (size_t)n_samples, P.fft_size, trim, n_trim, h);
    std::vector<double> seg((size_t)target + 1);
    float mf_max = -7.0f;
    GfwOptimArgs &A = emu_oA;
    memset(&A, 0, sizeof(A));
    A.gyro = (const float *)(h + L.o_gyro); A.win = (const float *)(h + L.o_win); A.cs = (const float2 *)(h + L.o_cs); A.trim = (const double *)(h + L.o_trim);
    A.lf = lf; A.mf = mf; A.hf = hf; A.mf_max = &mf_max; A.rank = rank; A.masked = masked; A.rank_nms = rank_nms; A.seg_ms = seg.data(); A.points_ms = points_ms; A.n_points = n_points;
    A.sample_rate = sample_rate; A.ratio = P.ratio; A.total_duration = P.total_duration; A.scale = P.scale;
    A.n_samples = (int32_t)n_samples; A.fft_size = P.fft_size; A.n_windows = P.n_windows; A.n_trim = n_trim; A.target = target;
    A.segment_size = P.segment_size; A.nms_radius = P.nms_radius;
    for (int i = 0; i < 4; ++i) A.bin[i] = P.bin[i];
    const int wgs = (P.n_windows + GFW_OPTIM_LANES - 1) / GFW_OPTIM_LANES;
    int rc = 0;
    if (P.n_windows > 0) {                                                    // gfw_launch_optim_spectrum, gfw_launch_optim_rank: zero-sized launches are skipped
        rc = emu::run_grid(P.n_windows, emu_optim_spectrum_body);
        if (!rc) rc = emu::run_grid(1, emu_optim_max_body);
        if (!rc) rc = emu::run_grid(wgs, emu_optim_rank_body);
    }
    if (rc || !points || target <= 0) return rc;
    if (P.n_windows > 0) rc = emu::run_grid(wgs, emu_optim_nms_body);         // gfw_launch_optim_points
    if (!rc) rc = emu::run_grid(target, emu_optim_pick_body);
    if (!rc) rc = emu::run_grid(1, emu_optim_gather_body);
    return rc;
}
