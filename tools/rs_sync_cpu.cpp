// rs_sync_cpu.cpp — the rs-sync search's cost arithmetic (gyroflow_amd/csrc/gfw_sync_rs.h) as a single-threaded loop on the host, for tools/rs_sync_bench.py: the
// range costs of a few candidates over prepared points (bearings and times as the prepare stage leaves them), in the kernel's own order — 64 lane-strided partial
// sums, then the butterfly — so that the costs can be compared with the device's to the bit.  Built with the host pass of hipcc only; not part of the library.
//   rs_sync_cpu <dump>   dump: int32 (n_track, n_ranges, n_pairs, total, n_cand, hypotheses, refits, sweeps), f64 loss_scale, track_t [n_track], track_q [n_track][4],
//                        int32 range_first [n_ranges + 1], pair_first [n_pairs + 1], f64 prep [2][total][4], candidates [n_cand]
//   prints the seconds of the loop, then n_ranges x n_cand costs as C hex floats
#include <chrono>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../include/gfwarp.h"
#include "../gyroflow_amd/csrc/gfw_sync_rs.h"

static double wave_sum(double *v) {                                          // v[64] -> the butterfly's sum (every lane ends with it: lane 0's is returned)
    for (int off = 32; off > 0; off >>= 1) {
        double w[64];
        for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; ++l) v[l] = w[l];
    }
    return v[0];
}
static double score(const std::vector<double> &m, int n, double k, const double *t) {
    double acc[64] = {0.0};
    for (int i = 0; i < n; ++i) { const double x2 = gfw_rs_residual2(k, m[i * 3], m[i * 3 + 1], m[i * 3 + 2], t); acc[i & 63] = acc[i & 63] + (x2 / (1.0 + x2)); }
    return wave_sum(acc);
}
static void fit(const std::vector<double> &m, int n, double k, bool weighted, int sweeps, double *t) {
    double acc[6][64] = {{0.0}};
    for (int i = 0; i < n; ++i) {
        const double m0 = m[i * 3], m1 = m[i * 3 + 1], m2 = m[i * 3 + 2];
        double w = 1.0;
        if (weighted) { const double x2 = gfw_rs_residual2(k, m0, m1, m2, t); w = 1.0 / ((1.0 + x2) * (1.0 + x2)); }
        const double p[6] = {m0 * m0, m0 * m1, m0 * m2, m1 * m1, m1 * m2, m2 * m2};
        for (int j = 0; j < 6; ++j) acc[j][i & 63] = acc[j][i & 63] + (weighted ? w * p[j] : p[j]);
    }
    double G[6];
    for (int j = 0; j < 6; ++j) G[j] = wave_sum(acc[j]);
    gfw_rs_smallest(G, sweeps, t);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: rs_sync_cpu <dump>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[8];
    double loss_scale = 0.0;
    bool ok = fread(head, sizeof(head), 1, f) == 1 && fread(&loss_scale, 8, 1, f) == 1;
    const int n_track = head[0], n_ranges = head[1], n_pairs = head[2], total = head[3], n_cand = head[4], hypotheses = head[5], refits = head[6], sweeps = head[7];
    std::vector<double> T((size_t)n_track), Q((size_t)n_track * 4), prep((size_t)total * 8), cand((size_t)n_cand);
    std::vector<int32_t> range_first((size_t)n_ranges + 1), pair_first((size_t)n_pairs + 1);
    ok = ok && fread(T.data(), 8, T.size(), f) == T.size() && fread(Q.data(), 8, Q.size(), f) == Q.size();
    ok = ok && fread(range_first.data(), 4, range_first.size(), f) == range_first.size() && fread(pair_first.data(), 4, pair_first.size(), f) == pair_first.size();
    ok = ok && fread(prep.data(), 8, prep.size(), f) == prep.size() && fread(cand.data(), 8, cand.size(), f) == cand.size();
    fclose(f);
    if (!ok) { fprintf(stderr, "short dump\n"); return 2; }
    std::vector<double> costs((size_t)n_ranges * n_cand), m;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < n_ranges; ++r) {
        for (int c = 0; c < n_cand; ++c) {
            double sum = 0.0;
            for (int p = range_first[r]; p < range_first[r + 1]; ++p) {
                const int first = pair_first[p], n = pair_first[p + 1] - first;
                double cost = 0.0;
                if (n > 0) {
                    m.resize((size_t)n * 3);
                    for (int i = 0; i < n; ++i)
                        gfw_rs_moment_vector(T.data(), Q.data(), n_track, 0, n_track - 1, prep.data() + (size_t)(first + i) * 4, prep.data() + ((size_t)total + first + i) * 4, cand[c], &m[(size_t)i * 3]);
                    double t[3];
                    fit(m, n, loss_scale, false, sweeps, t);
                    double best = score(m, n, loss_scale, t);
                    if (n >= 2) {
                        for (int h = 1; h <= hypotheses; ++h) {
                            const int i = (7 * h) % n, j = (13 * h + 5) % n;
                            double x[3];
                            gfw_pe_cross(&m[(size_t)i * 3], &m[(size_t)j * 3], x);
                            const double len2 = ((x[0] * x[0]) + (x[1] * x[1])) + (x[2] * x[2]);
                            if (!(len2 > 0.0)) continue;
                            const double len = __builtin_sqrt(len2);
                            const double th[3] = {x[0] / len, x[1] / len, x[2] / len};
                            const double s = score(m, n, loss_scale, th);
                            if (s < best) { best = s; t[0] = th[0]; t[1] = th[1]; t[2] = th[2]; }
                        }
                    }
                    for (int k = 0; k < refits; ++k) fit(m, n, loss_scale, true, sweeps, t);
                    cost = score(m, n, loss_scale, t);
                }
                sum = sum + cost;
            }
            costs[(size_t)r * n_cand + c] = sum;
        }
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%.6f\n", seconds);
    for (double c : costs) printf("%a\n", c);
    return 0;
}
