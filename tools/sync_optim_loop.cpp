// tools/sync_optim_loop.cpp — the helper of tools/sync_optim_bench.py and of tests/test_sync_optim_loop.py: the choice of a clip's sync points (optimsync.rs:68-225) in
// its f32 form as a plain single-threaded C++ loop on the host — per window and bin a sequential fold over the samples, then the
// reference's own loops for the rank, the masks, the suppression and the picks.  Context for the device call's time, and a second statement of its results (compared
// to the bit).  Tables, resampling and the derived sizes are the library's host-only helpers (gfw_sync_optim_host.h).  Build with -O2 -ffp-contract=off; with
// -DSYNC_OPTIM_LOOP_MAIN the file is a stand-alone program (for sanitizer builds): `sync_optim_loop DUMP` reads a dump written by the test, resamples, runs, and
// prints the points and a checksum of the ranks.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../gyroflow_amd/csrc/gfw_sync_optim_host.h"

static float nlfunc(float arg, float trip_point) { return arg < trip_point ? 0.0f : arg - trip_point; }

// gyro [3][n_samples] f64.  max_windows >= 0: only the band energies of the first max_windows windows (the bench's prefix of a long clip); < 0: everything.
// lf / mf / hf / rank / rank_nms [n_windows] f32, points_ms [target].  -> the number of points (or, for a prefix, 0)
extern "C" int sync_optim_loop(const double *gyro, long long n_samples, double sample_rate, int target, const double *trim, int n_trim, long long max_windows,
                               float *lf, float *mf, float *hf, float *rank, float *rank_nms, double *points_ms) {
    const GfwOptimShape P = gfw_optim_shape(n_samples, sample_rate, target);
    const int N = P.fft_size, H = N / 2;
    long long W = P.n_windows;
    const bool prefix = max_windows >= 0 && max_windows < W;
    if (prefix) W = max_windows;
    std::vector<float> win((size_t)N), c((size_t)N), s((size_t)N), xw((size_t)N * 3), spec((size_t)(H + 1) * 6), merged((size_t)H);
    gfw_optim_tables_host(N, win.data(), c.data(), s.data());
    for (long long w = 0; w < W; ++w) {
        for (int a = 0; a < 3; ++a)
            for (int n = 0; n < N; ++n) xw[(size_t)a * N + n] = (float)gyro[(size_t)a * n_samples + (size_t)w * 16 + n] * win[n];
        for (int k = 0; k <= H; ++k) {
            for (int a = 0; a < 3; ++a) {
                float re = 0.0f, im = 0.0f;
                int idx = 0;
                const float *x = xw.data() + (size_t)a * N;
                for (int n = 0; n < N; ++n) {
                    re = re + x[n] * c[idx];
                    im = im + (-(x[n] * s[idx]));
                    idx += k;
                    if (idx >= N) idx -= N;
                }
                spec[(size_t)k * 6 + 2 * a] = re; spec[(size_t)k * 6 + 2 * a + 1] = im;
            }
        }
        for (int k = 0; k < H; ++k) {
            float m[3];
            for (int a = 0; a < 3; ++a) {
                const float sr = spec[(size_t)k * 6 + 2 * a] + spec[(size_t)(k + 1) * 6 + 2 * a], si = spec[(size_t)k * 6 + 2 * a + 1] + (-spec[(size_t)(k + 1) * 6 + 2 * a + 1]);
                m[a] = sqrtf(sr * sr + si * si) * P.scale;
            }
            merged[k] = (m[0] + m[1]) + m[2];
        }
        float *bands[3] = {lf, mf, hf};
        for (int b = 0; b < 3; ++b) {
            float sum = 0.0f;
            for (int k = P.bin[b]; k < P.bin[b + 1]; ++k) sum = sum + merged[k];
            bands[b][w] = sum;
        }
    }
    if (prefix) return 0;
    float mf_max = 0.0f;
    for (long long i = 0; i < W; ++i) mf_max = fmaxf(mf_max, mf[i]);
    const bool low_motion = mf_max < 50.0f;
    std::vector<float> masked((size_t)W);
    for (long long i = 0; i < W; ++i) {
        rank[i] = low_motion ? (lf[i] + mf[i]) / (1.0f + nlfunc(hf[i], 450.0f) * 0.003f)
                             : mf[i] / (1.0f + nlfunc(hf[i], 450.0f) * 0.003f) / (1.0f + nlfunc(lf[i], 650.0f) * 0.003f);
        const double time = (double)i * P.ratio;
        bool inside = false;
        for (int q = 0; q < n_trim; ++q) inside = inside || (time >= trim[2 * q] && time <= trim[2 * q + 1]);
        masked[i] = (rank[i] < 50.0f || !inside) ? 0.0f : rank[i];
    }
    if (P.total_duration > 12.0)
        for (long long i = 0; i < W; ++i) {
            const double time = (double)i * P.ratio;
            if (time < 2.0 || time >= (P.total_duration - 2.0)) masked[i] = 0.0f;
        }
    for (long long i = 0; i < W; ++i) rank_nms[i] = masked[i];
    for (long long i = 0; i < W; ++i) {                                                // the reference's double loop as it stands (:173-179)
        const long long j0 = i - P.nms_radius > 0 ? i - P.nms_radius : 0, j1 = i + P.nms_radius < W - 1 ? i + P.nms_radius : W - 1;
        for (long long j = j0; j < j1; ++j)
            if (masked[j] < masked[i]) rank_nms[j] = 0.0f;
    }
    int n_points = 0;
    for (int i = 0; i < target; ++i) {
        const long long start = (long long)i * P.segment_size, end = start + P.segment_size < W ? start + P.segment_size : W;
        if (start >= end) continue;
        long long best = start;
        for (long long q = start; q < end; ++q)
            if (!(rank_nms[best] > rank_nms[q])) best = q;                             // max_by: the last maximal element
        if (rank_nms[best] < 0.1f) continue;
        points_ms[n_points++] = ((double)best * 16.0 + (double)N / 2.0) / sample_rate * 1000.0;
    }
    return n_points;
}

#ifdef SYNC_OPTIM_LOOP_MAIN
// DUMP: int64 n, int64 target, int64 n_trim, then f64 timestamps_ms [n], xyz [n][3], trim [n_trim][2]
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: sync_optim_loop DUMP\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[3];
    if (fread(head, 8, 3, f) != 3 || head[0] < 1) return 2;
    const int n = (int)head[0], target = (int)head[1], n_trim = (int)head[2];
    std::vector<double> ts((size_t)n), xyz((size_t)n * 3), trim((size_t)n_trim * 2 + 1);
    if (fread(ts.data(), 8, (size_t)n, f) != (size_t)n || fread(xyz.data(), 8, (size_t)n * 3, f) != (size_t)n * 3 || fread(trim.data(), 8, (size_t)n_trim * 2, f) != (size_t)n_trim * 2) return 2;
    fclose(f);
    double rate = 0.0;
    const unsigned long long S = gfw_optim_resample_count(ts.data(), nullptr, n, &rate);
    std::vector<double> gyro((size_t)S * 3 + 1);
    gfw_optim_resample_host(ts.data(), xyz.data(), nullptr, n, rate, S, gyro.data(), (size_t)S);
    const GfwOptimShape P = gfw_optim_shape((long long)S, rate, target);
    const size_t W = (size_t)P.n_windows;
    std::vector<float> lf(W + 1), mf(W + 1), hf(W + 1), rank(W + 1), nms(W + 1);
    std::vector<double> pts((size_t)target + 1);
    const int np = sync_optim_loop(gyro.data(), (long long)S, rate, target, trim.data(), n_trim, -1, lf.data(), mf.data(), hf.data(), rank.data(), nms.data(), pts.data());
    uint64_t sum = 1469598103934665603ull;                                             // FNV-1a over the ranks' bits
    for (size_t i = 0; i < W; ++i) { uint32_t b; memcpy(&b, &rank[i], 4); for (int k = 0; k < 4; ++k) { sum ^= (b >> (8 * k)) & 255u; sum *= 1099511628211ull; } }
    printf("rate %a samples %llu windows %zu rank_fnv %016llx points %d", rate, S, W, (unsigned long long)sum, np);
    for (int i = 0; i < np; ++i) printf(" %a", pts[i]);
    printf("\n");
    return 0;
}
#endif
