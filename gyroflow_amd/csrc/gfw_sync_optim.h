// gfw_sync_optim.h — the choice of a clip's sync points on the device (gfw_sync_optim.hip): OptimSync::run of src/core/synchronization/optimsync.rs:68-225 — the
// Blackman-windowed spectrogram of the gyro series, its band energies, the rank, the masks, the non-maximum suppression and one pick per segment
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gfwarp.h"

#define GFW_OPTIM_LANES 256             // lanes of a workgroup of every kernel
#define GFW_OPTIM_HOP 16                // step_size_samples (:79)
#define GFW_OPTIM_FFT_MIN 16            // fft_size = round(sample_rate) a call takes
#define GFW_OPTIM_FFT_MAX 8192
#define GFW_OPTIM_SAMPLES_MAX (1 << 24) // gyro samples of a call
#define GFW_OPTIM_TARGET_MAX 65535      // target_sync_points: a segment is a workgroup of the pick stage
#define GFW_OPTIM_TRIM_MAX 1024         // trim ranges

// LDS of a spectrum workgroup behind its static part: the windowed samples [fft_size] float4 (x, y, z, -) and the merged bins [fft_size / 2] f32
__host__ __device__ inline size_t gfw_optim_lds_bytes(int fft_size) { return (size_t)fft_size * 16 + (size_t)(fft_size / 2) * 4; }

struct GfwOptimArgs {
    const float *gyro;                  // [3][n_samples]: `x as f32` of every axis (device)
    const float *win;                   // [fft_size] blackman(fft_size)
    const float2 *cs;                   // [fft_size] (cos, sin)(2 pi j / fft_size): built in f64, rounded once
    const double *trim;                 // [n_trim][2] seconds
    float *lf, *mf, *hf;                // [n_windows] band energies
    float *mf_max;                      // [1] fold(0.0, f32::max) of mf
    float *rank;                        // [n_windows] before the masks
    float *masked;                      // [n_windows] behind them
    float *rank_nms;                    // [n_windows]
    double *seg_ms;                     // [target] the pick of a segment as a time, -1.0 = none
    double *points_ms;                  // [target] the picks that exist, in segment order
    int32_t *n_points;
    double sample_rate, ratio, total_duration;
    float scale;                        // (1.0 / fft_size as f32).sqrt() / fft_size as f32 * 256.0 (:83)
    int32_t n_samples, fft_size, n_windows, n_trim, target, segment_size, nms_radius;
    int32_t bin[4];                     // map_to_bin of 0, 2, 30, 2000 Hz (:108-113)
};
// Zero-sized launches are skipped.  spectrum: -> lf, mf, hf; rank: -> mf_max, rank, masked (two launches); points: -> rank_nms, seg_ms, points_ms, n_points (three launches)
hipError_t gfw_launch_optim_spectrum(const GfwOptimArgs &A, hipStream_t s);
hipError_t gfw_launch_optim_rank(const GfwOptimArgs &A, hipStream_t s);
hipError_t gfw_launch_optim_points(const GfwOptimArgs &A, hipStream_t s);
