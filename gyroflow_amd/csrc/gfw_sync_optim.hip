// gfw_sync_optim.hip — where in a clip to sync (OptimSync::run, src/core/synchronization/optimsync.rs:68-225).
//
// The reference takes a Blackman-windowed forward transform of round(sample_rate) gyro samples per axis every 16 samples (rustfft, f32), folds every bin with its
// mirror (`zip(cm.iter(), cm.iter().rev())`: X[k] + X[N-1-k]), and from the norms' band sums makes a rank per window, masks it, suppresses non-maxima and picks one
// window per segment.  A transform library's summation order is no contract, so the quantity is restated: bin k of a window is the LEFT
// FOLD over n of xw[n] * c[(k n) mod N] (and of -(xw[n] * s[..])) in f32, one product and one sum at a time, the twiddles read from a table the host built in f64;
// X[N-1-k] of a real input is conj(X[k+1]), so half the spectrum is computed.  A fold that is sequential in n gives any launch shape the same bits; the
// parallelism is (window, bin, axis).
//
// Spectrum stage: a workgroup is a window with its three axes.  The windowed samples lie in LDS as float4 (one broadcast ds_read_b128 per n serves the three axes),
// a lane owns bins k = lane, lane + 256, ... and walks n with the incremental index idx += k (mod N by one compare): no multiply or modulo in the loop.  The
// twiddle pair of (n, k) is ONE 8-byte load from a table in GLOBAL memory (8 N bytes: L1 / L2 resident); 20 N bytes of tables and samples would be the whole LDS
// at N = 8192, and one form serves every size.  The bins of a round of 256 meet in LDS for the pair sums; the band folds run over the merged bins in index order
// on one lane per band — at most N / 2 additions beside a body of N * N / 2.
// Rank, mask, non-maximum suppression and the picks are a lane per window / a workgroup per segment; a call is six launches for any clip length.
// Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; every barrier sits in workgroup-uniform control flow.
#include <hip/hip_runtime.h>
#include "gfw_sync_optim.h"

#ifndef GFW_OPTIM_DYN_LDS                                                            // (the host interpreter has no dynamic LDS: it defines a static array of the largest size)
#define GFW_OPTIM_DYN_LDS(name) extern __shared__ float4 name[]
#endif

#define GFW_OPTIM_PICK_RESET (1 << 30)                                                 // pick stage: a lane's run held a NaN (rides in its s_idx)
__device__ __forceinline__ int gfw_optim_lane() { return (int)(threadIdx.y * 64u + threadIdx.x); }

// Spectrum stage: workgroup blockIdx.x is window blockIdx.x
__global__ __launch_bounds__(GFW_OPTIM_LANES) void gfw_optim_spectrum_kernel(const GfwOptimArgs A) {
    GFW_OPTIM_DYN_LDS(s_x);                                                          // [N] windowed samples, then [N / 2] merged bins
    __shared__ float s_spec[GFW_OPTIM_LANES + 1][6];                                 // the bins of a round: slot 0 = the last bin of the round before, slot 1 + lane = this round's
    const int t = gfw_optim_lane();
    const int N = A.fft_size, H = N / 2;
    const size_t w0 = (size_t)blockIdx.x * GFW_OPTIM_HOP;                            // windows(fft_size).step_by(16) (:93-94)
    float *s_merged = (float *)(s_x + N);
    for (int n = t; n < N; n += GFW_OPTIM_LANES) {
        const float win = A.win[n];
        const float *g = A.gyro + w0 + n;                                            // w0 + n <= n_samples - 1: the host counts the windows that fit
        s_x[n] = make_float4(g[0] * win, g[(size_t)A.n_samples] * win, g[(size_t)A.n_samples * 2] * win, 0.0f);
    }
    __syncthreads();
    const int rounds = (H + 1 + GFW_OPTIM_LANES - 1) / GFW_OPTIM_LANES;               // bins 0 .. H
    for (int j = 0; j < rounds; ++j) {
        const int k = j * GFW_OPTIM_LANES + t;
        float re0 = 0.0f, re1 = 0.0f, re2 = 0.0f, im0 = 0.0f, im1 = 0.0f, im2 = 0.0f;
        if (k <= H) {
            int idx = 0;                                                             // (k n) mod N
            for (int n = 0; n < N; ++n) {
                const float4 x = s_x[n];
                const float2 cs = A.cs[idx];
                re0 = re0 + x.x * cs.x; im0 = im0 + (-(x.x * cs.y));
                re1 = re1 + x.y * cs.x; im1 = im1 + (-(x.y * cs.y));
                re2 = re2 + x.z * cs.x; im2 = im2 + (-(x.z * cs.y));
                idx += k;
                if (idx >= N) idx -= N;
            }
            float *o = s_spec[1 + t];
            o[0] = re0; o[1] = im0; o[2] = re1; o[3] = im1; o[4] = re2; o[5] = im2;
        }
        __syncthreads();
        if (k >= 1 && k <= H) {                                                      // merged bin k - 1: X[k-1] + conj(X[k]) per axis, norm, scale, (x + y) + z (:98-101, :126-128)
            const float *a = s_spec[t];
            const float r0 = a[0] + re0, i0 = a[1] + (-im0), r1 = a[2] + re1, i1 = a[3] + (-im1), r2 = a[4] + re2, i2 = a[5] + (-im2);
            const float m0 = sqrtf(r0 * r0 + i0 * i0) * A.scale, m1 = sqrtf(r1 * r1 + i1 * i1) * A.scale, m2 = sqrtf(r2 * r2 + i2 * i2) * A.scale;
            s_merged[k - 1] = (m0 + m1) + m2;
        }
        __syncthreads();
        if (t == GFW_OPTIM_LANES - 1 && k <= H) {                                    // read by lane 0 behind the next round's first barrier
            float *o = s_spec[0];
            o[0] = re0; o[1] = im0; o[2] = re1; o[3] = im1; o[4] = re2; o[5] = im2;
        }
    }
    __syncthreads();
    if (t < 3) {                                                                     // bins[map_to_bin(begin)..map_to_bin(end)].iter().sum::<f32>() (:115-121): ends exclusive, bins <= H - 1
        float sum = 0.0f;
        for (int b = A.bin[t]; b < A.bin[t + 1]; ++b) sum = sum + s_merged[b];
        (t == 0 ? A.lf : t == 1 ? A.mf : A.hf)[blockIdx.x] = sum;
    }
}

// mf.iter().cloned().fold(0.0_f32, f32::max) (:136): one workgroup.  The maximum of numbers does not depend on the order
__global__ __launch_bounds__(GFW_OPTIM_LANES) void gfw_optim_max_kernel(const GfwOptimArgs A) {
    __shared__ float s_max[GFW_OPTIM_LANES];
    const int t = gfw_optim_lane();
    float m = 0.0f;
    for (int i = t; i < A.n_windows; i += GFW_OPTIM_LANES) m = fmaxf(m, A.mf[i]);
    s_max[t] = m;
    __syncthreads();
    if (t == 0) {
        for (int j = 1; j < GFW_OPTIM_LANES; ++j) m = fmaxf(m, s_max[j]);
        A.mf_max[0] = m;
    }
}

__device__ __forceinline__ float gfw_optim_nlfunc(float arg, float trip_point) { return arg < trip_point ? 0.0f : arg - trip_point; }     // :228-234

// The rank of a window and its masks (:139-170): a lane is a window
__global__ __launch_bounds__(GFW_OPTIM_LANES) void gfw_optim_rank_kernel(const GfwOptimArgs A) {
    const int i = (int)(blockIdx.x * (unsigned)GFW_OPTIM_LANES) + gfw_optim_lane();
    if (i >= A.n_windows) return;
    const float lf = A.lf[i], mf = A.mf[i], hf = A.hf[i];
    float r;
    if (A.mf_max[0] < 50.0f) r = (lf + mf) / (1.0f + gfw_optim_nlfunc(hf, 450.0f) * 0.003f);
    else r = mf / (1.0f + gfw_optim_nlfunc(hf, 450.0f) * 0.003f) / (1.0f + gfw_optim_nlfunc(lf, 650.0f) * 0.003f);
    A.rank[i] = r;
    const double time = (double)i * A.ratio;
    bool inside = false;                                                             // trim_ranges_s.iter().any(..): nothing is inside no range
    for (int q = 0; q < A.n_trim; ++q) inside = inside || (time >= A.trim[2 * q] && time <= A.trim[2 * q + 1]);
    if (r < 50.0f || !inside) r = 0.0f;
    if (A.total_duration > 12.0 && (time < 2.0 || time >= (A.total_duration - 2.0))) r = 0.0f;
    A.masked[i] = r;
}

// Non-maximum suppression (:172-179) as a windowed maximum: element j is cleared when some i with max(i - r, 0) <= j < min(i + r, len - 1) — that is
// j - r < i <= j + r, and j is not the last element — has rank[j] < rank[i].  Reads the masked rank only, as the reference reads `rank`, never `rank_nms`
__global__ __launch_bounds__(GFW_OPTIM_LANES) void gfw_optim_nms_kernel(const GfwOptimArgs A) {
    const int j = (int)(blockIdx.x * (unsigned)GFW_OPTIM_LANES) + gfw_optim_lane();
    const int len = A.n_windows;
    if (j >= len) return;
    const float own = A.masked[j];
    float out = own;
    if (j < len - 1) {
        const long long lo = (long long)j - A.nms_radius + 1, hi = (long long)j + A.nms_radius;
        const int i0 = lo < 0 ? 0 : (int)lo, i1 = hi > len - 1 ? len - 1 : (int)hi;
        for (int i = i0; i <= i1; ++i)
            if (own < A.masked[i]) { out = 0.0f; break; }
    }
    A.rank_nms[j] = out;
}

// One pick per segment (:182-204): workgroup blockIdx.x is a segment.  A lane folds a contiguous run, lane 0 the lanes' picks in lane order: together
// Iterator::max_by(partial_cmp(..).unwrap_or(Equal)) over the segment in index order — the sequential fold of `x > y ? x : y`, which keeps the LAST maximal element
// and which a NaN RESETS: nothing compares greater than a NaN and a NaN compares greater than nothing, so the fold's state behind a NaN is what a fold begun at that
// NaN would hold, whatever came before.  That operation is not associative, so a lane also reports whether its run held a NaN (bit 30 of s_idx: a segment has at
// most 2^20 windows), and lane 0 then REPLACES its running pick by that lane's instead of comparing — the value behind the NaN must not meet the earlier maximum
__global__ __launch_bounds__(GFW_OPTIM_LANES) void gfw_optim_pick_kernel(const GfwOptimArgs A) {
    __shared__ float s_val[GFW_OPTIM_LANES];
    __shared__ int s_idx[GFW_OPTIM_LANES];
    const int t = gfw_optim_lane();
    const long long start = (long long)blockIdx.x * A.segment_size;
    const long long stop = start + A.segment_size < A.n_windows ? start + A.segment_size : A.n_windows;
    const int n = stop > start ? (int)(stop - start) : 0;                            // a segment starting beyond the end yields nothing, as an empty one does
    const int run = (n + GFW_OPTIM_LANES - 1) / GFW_OPTIM_LANES;
    const int c0 = t * run < n ? t * run : n, c1 = c0 + run < n ? c0 + run : n;
    float best = 0.0f;
    int idx = -1, reset = 0;
    for (int c = c0; c < c1; ++c) {
        const float v = A.rank_nms[start + c];
        if (idx < 0 || !(best > v)) { best = v; idx = c; }                           // max_by: the later of equals (and of what does not compare)
        if (v != v) reset = GFW_OPTIM_PICK_RESET;
    }
    s_val[t] = best; s_idx[t] = idx < 0 ? idx : (idx | reset);
    __syncthreads();
    if (t == 0) {
        int pick = -1;
        float high = 0.0f;
        for (int j = 0; j < GFW_OPTIM_LANES; ++j) {
            const int at = s_idx[j];
            if (at < 0) continue;
            if (pick < 0 || (at & GFW_OPTIM_PICK_RESET) || !(high > s_val[j])) { high = s_val[j]; pick = at & (GFW_OPTIM_PICK_RESET - 1); }
        }
        double ms = -1.0;
        if (pick >= 0 && !(high < 0.1f)) ms = ((double)(start + pick) * 16.0 + (double)A.fft_size / 2.0) / A.sample_rate * 1000.0;       // :199
        A.seg_ms[blockIdx.x] = ms;
    }
}

// filter_map(..).collect(): the picks that exist, in segment order.  One workgroup; a lane owns a contiguous run of segments
__global__ __launch_bounds__(GFW_OPTIM_LANES) void gfw_optim_gather_kernel(const GfwOptimArgs A) {
    __shared__ int s_at[GFW_OPTIM_LANES];
    const int t = gfw_optim_lane();
    const int run = (A.target + GFW_OPTIM_LANES - 1) / GFW_OPTIM_LANES;
    const int c0 = t * run < A.target ? t * run : A.target, c1 = c0 + run < A.target ? c0 + run : A.target;
    int count = 0;
    for (int c = c0; c < c1; ++c) count += A.seg_ms[c] >= 0.0 ? 1 : 0;
    s_at[t] = count;
    __syncthreads();
    if (t == 0) {
        int at = 0;
        for (int j = 0; j < GFW_OPTIM_LANES; ++j) { const int m = s_at[j]; s_at[j] = at; at += m; }
        A.n_points[0] = at;
    }
    __syncthreads();
    int at = s_at[t];
    for (int c = c0; c < c1; ++c) {
        const double ms = A.seg_ms[c];
        if (ms >= 0.0) A.points_ms[at++] = ms;
    }
}

#ifndef GFW_HOST_INTERPRETER                                                         // (the interpreter is its own launcher)
static const dim3 kOptimBlock(64, GFW_OPTIM_LANES / 64);
hipError_t gfw_launch_optim_spectrum(const GfwOptimArgs &A, hipStream_t s) {
    if (A.n_windows <= 0) return hipSuccess;
    const size_t lds = gfw_optim_lds_bytes(A.fft_size);
    if (lds > 48 * 1024) {                                                           // above the default limit of dynamic LDS a kernel has to be told
        const hipError_t e = hipFuncSetAttribute((const void *)gfw_optim_spectrum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gfw_optim_spectrum_kernel, dim3((unsigned)A.n_windows), kOptimBlock, lds, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_optim_rank(const GfwOptimArgs &A, hipStream_t s) {
    if (A.n_windows <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_optim_max_kernel, dim3(1), kOptimBlock, 0, s, A);
    hipLaunchKernelGGL(gfw_optim_rank_kernel, dim3((unsigned)((A.n_windows + GFW_OPTIM_LANES - 1) / GFW_OPTIM_LANES)), kOptimBlock, 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_optim_points(const GfwOptimArgs &A, hipStream_t s) {
    if (A.target <= 0) return hipSuccess;
    if (A.n_windows > 0) hipLaunchKernelGGL(gfw_optim_nms_kernel, dim3((unsigned)((A.n_windows + GFW_OPTIM_LANES - 1) / GFW_OPTIM_LANES)), kOptimBlock, 0, s, A);
    hipLaunchKernelGGL(gfw_optim_pick_kernel, dim3((unsigned)A.target), kOptimBlock, 0, s, A);
    hipLaunchKernelGGL(gfw_optim_gather_kernel, dim3(1), kOptimBlock, 0, s, A);
    return hipGetLastError();
}
#endif
