// gfw_api_sync_optim.inc — part of gfw_api.hip (textually included): the choice of a clip's sync points — gfw_optim_tables, gfw_optim_resample (host only),
// gfw_sync_optim_rank, gfw_sync_optim_points (gfw_sync_optim.hip).  What they stage and derive on the host is gfw_sync_optim_host.h's.

extern "C" int gfw_optim_tables(int fft_size, float *win, float *cosv, float *sinv) {
    if (fft_size < GFW_OPTIM_FFT_MIN || fft_size > GFW_OPTIM_FFT_MAX) { set_error("bad optim tables: fft_size %d, %d .. %d are served", fft_size, GFW_OPTIM_FFT_MIN, GFW_OPTIM_FFT_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    gfw_optim_tables_host(fft_size, win, cosv, sinv);
    return GFW_OK;
}

extern "C" int gfw_optim_resample(const double *timestamps_ms, const double *xyz, const uint8_t *has, int n, double *out, int64_t out_stride, int64_t *n_out, double *sample_rate) {
    if (n < 1 || !timestamps_ms || !xyz || !n_out || !sample_rate) { set_error("bad optim resample arguments (n %d: OptimSync::new is None without samples; or a null array)", n); return GFW_ERR_INVALID_ARGUMENT; }
    double sr = 0.0;
    const unsigned long long count = gfw_optim_resample_count(timestamps_ms, has, n, &sr);
    if (count > (unsigned long long)GFW_OPTIM_SAMPLES_MAX) { set_error("the series resamples to %llu samples (rate %g): at most %d", count, sr, GFW_OPTIM_SAMPLES_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    if (out && out_stride < (int64_t)count) { set_error("the series resamples to %llu samples: out_stride %lld is too small", count, (long long)out_stride); return GFW_ERR_INVALID_ARGUMENT; }
    if (out) gfw_optim_resample_host(timestamps_ms, xyz, has, n, sr, count, out, (size_t)out_stride);
    *n_out = (int64_t)count; *sample_rate = sr;
    return GFW_OK;
}

// One body serves both entries: `points` false = gfw_sync_optim_rank (three launches), true = gfw_sync_optim_points (six).
struct OptimOut { float *lf, *mf, *hf, *rank, *rank_nms; double *points_ms; int32_t *n_points; int32_t *n_windows; double *ratio; };
static int sync_optim_impl(gfw_ctx *c, const double *gyro, int64_t n_samples, double sample_rate, bool points, int target, const double *trim, int n_trim,
                           const OptimOut &out, int out_on_device) {
    if (!c || n_samples < 0 || n_trim < 0) { set_error("bad optim arguments (null context, or a negative count)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!std::isfinite(sample_rate) || sample_rate <= 0.0) { set_error("bad optim arguments: sample_rate %g", sample_rate); return GFW_ERR_INVALID_ARGUMENT; }
    const unsigned long long fft = gfw_optim_fft_size(sample_rate);
    if (fft < GFW_OPTIM_FFT_MIN || fft > GFW_OPTIM_FFT_MAX) { set_error("sample_rate %g: fft_size %llu, %d .. %d are served", sample_rate, fft, GFW_OPTIM_FFT_MIN, GFW_OPTIM_FFT_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_samples > GFW_OPTIM_SAMPLES_MAX) { set_error("%lld gyro samples: at most %d in a call", (long long)n_samples, GFW_OPTIM_SAMPLES_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_samples && !gyro) { set_error("bad optim arguments (%lld samples without their array)", (long long)n_samples); return GFW_ERR_INVALID_ARGUMENT; }
    if (points) {
        if (target < 1 || target > GFW_OPTIM_TARGET_MAX) { set_error("target_sync_points %d: 1 .. %d", target, GFW_OPTIM_TARGET_MAX); return GFW_ERR_INVALID_ARGUMENT; }
        if (n_trim > GFW_OPTIM_TRIM_MAX) { set_error("%d trim ranges: at most %d", n_trim, GFW_OPTIM_TRIM_MAX); return GFW_ERR_INVALID_ARGUMENT; }
        if (n_trim && !trim) { set_error("bad optim arguments (%d trim ranges without their array)", n_trim); return GFW_ERR_INVALID_ARGUMENT; }
        if (!out.points_ms || !out.n_points) { set_error("bad optim arguments (a null points_ms or n_points)"); return GFW_ERR_INVALID_ARGUMENT; }
    } else { target = 0; n_trim = 0; }
    const GfwOptimShape P = gfw_optim_shape(n_samples, sample_rate, target);
    const size_t W = (size_t)P.n_windows;
    API_TRY(enter_device(c));
    // the series as f32, the tables and the trim ranges through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    const GfwOptimLayout L = gfw_optim_layout((size_t)n_samples, P.fft_size, n_trim);
    StagedBlock B;
    HIP_TRY(c->optim_ring.acquire(L.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_optim_fill(L, gyro, (size_t)n_samples, P.fft_size, trim, n_trim, B.h());
    HIP_TRY(B.upload(L.total, c->stream), GFW_ERR_HIP);
    CallOutputs O(c->d_out, out_on_device);
    int o_a, o_b, o_c, o_d;
    if (points) { o_a = O.add(out.points_ms, 8 * (size_t)target); o_b = O.add(out.n_points, 4); o_c = O.add(out.rank, 4 * W); o_d = O.add(out.rank_nms, 4 * W); }
    else { o_a = O.add(out.lf, 4 * W); o_b = O.add(out.mf, 4 * W); o_c = O.add(out.hf, 4 * W); o_d = O.add(out.rank, 4 * W); }
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    // outputs the caller does not ask for, and what only the kernels see, live in the work space: six f32 arrays of a window each, the maximum, the segments' picks
    const size_t wb = (4 * W + 7) / 8 * 8;
    HIP_TRY(c->d_sync_work.ensure(6 * wb + 8 + 8 * (size_t)target + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    GfwOptimArgs A;
    memset(&A, 0, sizeof(A));
    A.gyro = (const float *)(B.d() + L.o_gyro); A.win = (const float *)(B.d() + L.o_win); A.cs = (const float2 *)(B.d() + L.o_cs); A.trim = (const double *)(B.d() + L.o_trim);
    float *w_lf = (float *)wk, *w_mf = (float *)(wk + wb), *w_hf = (float *)(wk + 2 * wb), *w_rank = (float *)(wk + 3 * wb), *w_nms = (float *)(wk + 5 * wb);
    A.masked = (float *)(wk + 4 * wb); A.mf_max = (float *)(wk + 6 * wb); A.seg_ms = (double *)(wk + 6 * wb + 8);
    if (points) {
        A.lf = w_lf; A.mf = w_mf; A.hf = w_hf;
        A.points_ms = (double *)O.dev(o_a); A.n_points = (int32_t *)O.dev(o_b);
        A.rank = O.dev(o_c) ? (float *)O.dev(o_c) : w_rank; A.rank_nms = O.dev(o_d) ? (float *)O.dev(o_d) : w_nms;
    } else {
        A.lf = O.dev(o_a) ? (float *)O.dev(o_a) : w_lf; A.mf = O.dev(o_b) ? (float *)O.dev(o_b) : w_mf; A.hf = O.dev(o_c) ? (float *)O.dev(o_c) : w_hf;
        A.rank = O.dev(o_d) ? (float *)O.dev(o_d) : w_rank; A.rank_nms = w_nms;
    }
    A.sample_rate = sample_rate; A.ratio = P.ratio; A.total_duration = P.total_duration; A.scale = P.scale;
    A.n_samples = (int32_t)n_samples; A.fft_size = P.fft_size; A.n_windows = P.n_windows; A.n_trim = n_trim; A.target = target;
    A.segment_size = P.segment_size; A.nms_radius = P.nms_radius;
    for (int i = 0; i < 4; ++i) A.bin[i] = P.bin[i];
    HIP_TRY(gfw_launch_optim_spectrum(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_optim_rank(A, c->stream), GFW_ERR_HIP);
    if (points) HIP_TRY(gfw_launch_optim_points(A, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);                          // behind the last launch that reads the slot's device side
    c->last_backend = points ? "sync_optim_points" : "sync_optim_rank";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    if (out.n_windows) *out.n_windows = P.n_windows;                        // what the arguments alone decide: the caller's host memory, whatever out_on_device says
    if (out.ratio) *out.ratio = P.ratio;
    return GFW_OK;
}
extern "C" int gfw_sync_optim_rank(gfw_ctx *c, const double *gyro, int64_t n_samples, double sample_rate, float *lf, float *mf, float *hf, float *rank,
                                   int32_t *n_windows, int out_on_device) {
    const OptimOut out = {lf, mf, hf, rank, nullptr, nullptr, nullptr, n_windows, nullptr};
    return sync_optim_impl(c, gyro, n_samples, sample_rate, false, 0, nullptr, 0, out, out_on_device);
}
extern "C" int gfw_sync_optim_points(gfw_ctx *c, const double *gyro, int64_t n_samples, double sample_rate, int target_sync_points, const double *trim_ranges_s, int n_trim,
                                     double *points_ms, int32_t *n_points, float *rank, float *rank_nms, double *ratio, int out_on_device) {
    const OptimOut out = {nullptr, nullptr, nullptr, rank, rank_nms, points_ms, n_points, nullptr, ratio};
    return sync_optim_impl(c, gyro, n_samples, sample_rate, true, target_sync_points, trim_ranges_s, n_trim, out, out_on_device);
}
