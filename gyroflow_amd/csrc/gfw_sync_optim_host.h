// gfw_sync_optim_host.h — host only, no HIP and no context: what gfw_sync_optim_rank / gfw_sync_optim_points stage for the kernels of gfw_sync_optim.hip, the tables
// behind gfw_optim_tables and the resampling behind gfw_optim_resample (OptimSync::new).  Included by gfw_api.hip, by the interpreter's driver and by stand-alone host
// programs; the kernels' translation unit does not see it.  Compile with -ffp-contract=off: the window is the reference's f32 arithmetic, one operation at a time.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "gfw_layout.h"

// `v as usize` of a double (Rust: truncating, saturating, NaN -> 0), capped at 2^62
inline unsigned long long gfw_optim_as_usize(double v) {
    if (!(v >= 1.0)) return 0ull;
    if (v >= 4611686018427387904.0) return 1ull << 62;
    return (unsigned long long)v;
}
// `sample_rate.round() as usize` (:82): half away from zero, as round() rounds
inline unsigned long long gfw_optim_fft_size(double sample_rate) { return gfw_optim_as_usize(round(sample_rate)); }
// windows(fft_size).step_by(16) (:93-94)
inline long long gfw_optim_windows(long long n_samples, long long fft_size) { return n_samples < fft_size || fft_size < 1 ? 0 : (n_samples - fft_size) / 16 + 1; }

// blackman(width) as written (optimsync.rs:15-27): f32 arithmetic, the host's cosf, size = width - 1 — and the twiddles (cos, sin)(2 pi j / width), evaluated in f64
// and rounded once.  Any of the three arrays may be null.
inline void gfw_optim_tables_host_one(int width, int i, float *win, float *cosv, float *sinv) {
    const float pi = 3.14159274101257324f;                                           // std::f32::consts::PI
    const float a0 = 7938.0f / 18608.0f, a1 = 9240.0f / 18608.0f, a2 = 1430.0f / 18608.0f;
    const float size = (float)(width - 1), n = (float)i;
    const float c1 = cosf(2.0f * pi * n / size), c2 = cosf(4.0f * pi * n / size);
    const float p1 = a1 * c1, p2 = a2 * c2;
    const float d = a0 - p1;
    *win = d + p2;
    const double ang = 2.0 * 3.14159265358979323846 * (double)i / (double)width;
    *cosv = (float)cos(ang); *sinv = (float)sin(ang);
}
inline void gfw_optim_tables_host(int width, float *win, float *cosv, float *sinv) {
    for (int i = 0; i < width; ++i) {
        float w, c, s;
        gfw_optim_tables_host_one(width, i, &w, &c, &s);
        if (win) win[i] = w;
        if (cosv) cosv[i] = c;
        if (sinv) sinv[i] = s;
    }
}

// OptimSync::new (optimsync.rs:30-66): the gyro resampled at its average rate.  timestamps_ms [n], xyz [n][3], has [n] (0 = `gyro: None`, which counts as (0, 0, 0)
// where it is interpolated — unwrap_or_default — and does not count for the rate; nullptr = all present).  -> the number of samples `(duration_ms * avg_sr / 1000.0)
// as usize`; `out` (nullptr, or [3][stride] with stride >= that number) receives axis a at out + a * stride.  n >= 1.
inline unsigned long long gfw_optim_resample_count(const double *ts, const uint8_t *has, int n, double *sample_rate) {
    const double duration_ms = ts[n - 1] - ts[0];
    long long present = 0;
    for (int i = 0; i < n; ++i) present += (!has || has[i]) ? 1 : 0;
    const double avg_sr = (double)present / duration_ms * 1000.0;
    *sample_rate = avg_sr;
    return gfw_optim_as_usize(duration_ms * avg_sr / 1000.0);
}
inline void gfw_optim_resample_host(const double *ts, const double *xyz, const uint8_t *has, int n, double avg_sr, unsigned long long count, double *out, size_t stride) {
    static const double none[3] = {0.0, 0.0, 0.0};
    for (unsigned long long i = 0; i < count; ++i) {
        const double t = (double)i * 1000.0 / avg_sr;
        int lo = 0, hi = n;                                                          // partition_point(|sample| sample.timestamp_ms < t)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (ts[mid] < t) lo = mid + 1; else hi = mid;
        }
        const int i_r = lo < n - 1 ? lo : n - 1, i_l = (i_r > 1 ? i_r : 1) - 1;
        const double *l = (!has || has[i_l]) ? xyz + (size_t)i_l * 3 : none, *r = (!has || has[i_r]) ? xyz + (size_t)i_r * 3 : none;
        for (int a = 0; a < 3; ++a) {
            double v = l[a];
            if (i_l != i_r) v = (l[a] * (ts[i_r] - t) + r[a] * (t - ts[i_l])) / (ts[i_r] - ts[i_l]);
            out[(size_t)a * stride + (size_t)i] = v;
        }
    }
}

// What a call derives from (n_samples, sample_rate, target, n_trim) on the host, in the reference's own arithmetic
struct GfwOptimShape {
    int fft_size, n_windows, nms_radius, segment_size, bin[4];
    float scale;
    double ratio, total_duration;
};
inline int gfw_optim_map_to_bin(int fft_size, double sample_rate, double freq) {     // :108-113
    double b = round((double)fft_size / sample_rate * freq);
    if (!(b > 0.0)) b = 0.0;                                                         // .max(0.0)
    const double top = (double)(fft_size / 2 - 1);
    if (b > top) b = top;
    return (int)b;
}
inline GfwOptimShape gfw_optim_shape(long long n_samples, double sample_rate, int target) {
    GfwOptimShape P;
    P.fft_size = (int)gfw_optim_fft_size(sample_rate);
    P.n_windows = (int)gfw_optim_windows(n_samples, P.fft_size);
    P.nms_radius = (int)gfw_optim_as_usize((sample_rate / 16.0 / 2.0) * 8.0);        // :80
    const float fs = (float)P.fft_size;
    P.scale = sqrtf(1.0f / fs) / fs * 256.0f;                                        // :83
    const double freqs[4] = {0.0, 2.0, 30.0, 2000.0};
    for (int i = 0; i < 4; ++i) P.bin[i] = gfw_optim_map_to_bin(P.fft_size, sample_rate, freqs[i]);
    P.ratio = 16.0 / sample_rate;                                                    // :153
    P.total_duration = (double)P.n_windows * P.ratio;                                // :162
    P.segment_size = target > 0 ? (int)(((long long)P.n_windows + target - 1) / target) : 0;      // :182
    return P;
}

// The staged block: the three axes as f32 [3][n_samples], the window [fft_size], the twiddle pairs [fft_size][2], the trim ranges [n_trim][2] f64
struct GfwOptimLayout { size_t o_gyro, o_win, o_cs, o_trim, total; };
inline GfwOptimLayout gfw_optim_layout(size_t n_samples, int fft_size, int n_trim) {
    BlockLayout L;
    GfwOptimLayout G;
    G.o_gyro = L.add(12 * n_samples); G.o_win = L.add(4 * (size_t)fft_size); G.o_cs = L.add(8 * (size_t)fft_size); G.o_trim = L.add(16 * (size_t)n_trim);
    G.total = L.total;
    return G;
}
// Fills the block at `h`: gyro [3][n_samples] f64 -> `x as f32` (:76), the tables, the trim ranges
inline void gfw_optim_fill(const GfwOptimLayout &L, const double *gyro, size_t n_samples, int fft_size, const double *trim, int n_trim, char *h) {
    float *g = (float *)(h + L.o_gyro);
    for (size_t i = 0; i < 3 * n_samples; ++i) g[i] = (float)gyro[i];
    float *win = (float *)(h + L.o_win), *cs = (float *)(h + L.o_cs);
    for (int i = 0; i < fft_size; ++i) {
        float c, s;
        gfw_optim_tables_host_one(fft_size, i, &win[i], &c, &s);
        cs[2 * i] = c; cs[2 * i + 1] = s;
    }
    if (n_trim) memcpy(h + L.o_trim, trim, 16 * (size_t)n_trim);
}
