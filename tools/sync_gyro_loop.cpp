// tools/sync_gyro_loop.cpp — the helper of tools/sync_gyro_bench.py: the gyro-match offset search (find_offset/essential_matrix.rs:50-75, :109-131) of every range
// as a plain single-threaded C++ loop on the host — a sorted key array per range, std::lower_bound per lookup, the two stages one after the other.  Context for
// the device call's time, and a second statement of its results (the bench compares them to the bit).  Built by the bench with g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

static unsigned long long key_of(double v) {
    if (!(v >= 1.0)) return 0ull;
    if (v >= 18446744073709551616.0) return 0xffffffffffffffffull;
    return (unsigned long long)v;
}
struct Tree { std::vector<unsigned long long> keys; std::vector<const double *> rows; std::vector<uint8_t> has; };
static double cost_of(double offs, const double *est, const uint8_t *est_has, int n, const Tree &t) {
    double sum = 0.0;
    int matches = 0;
    for (int j = 0; j < n; ++j) {
        const unsigned long long q = key_of((est[(size_t)j * 4] - offs) * 1000.0);
        const size_t at = (size_t)(std::lower_bound(t.keys.begin(), t.keys.end(), q) - t.keys.begin());
        if (at >= t.keys.size()) continue;
        if (!t.has[at] || (est_has && !est_has[j])) continue;
        const double *g = t.rows[at] + 1, *o = est + (size_t)j * 4 + 1;
        const double d0 = g[0] - o[0], d1 = g[1] - o[1], d2 = g[2] - o[2];
        matches += 1;
        sum += (d0 * d0) * 70.0;
        sum += (d1 * d1) * 70.0;
        sum += (d2 * d2) * 100.0;
    }
    return n > 0 && matches > n / 2 ? sum / (double)matches : 1.7976931348623157e308;
}
// results: [n_ranges][4] (coarse value, coarse cost, value, cost); a range without candidates keeps its zeros
extern "C" void sync_gyro_loop(const int32_t *est_first, const double *est, const uint8_t *est_has, const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has,
                               int n_ranges, double initial_offset, double search_size, double *results) {
    const size_t steps = (size_t)key_of(search_size) * 2;
    for (int r = 0; r < n_ranges; ++r) {
        std::vector<std::pair<unsigned long long, int>> order;
        for (int i = gyro_first[r]; i < gyro_first[r + 1]; ++i) order.emplace_back(key_of(gyro[(size_t)i * 4] * 1000.0), i);
        std::stable_sort(order.begin(), order.end(), [](const std::pair<unsigned long long, int> &a, const std::pair<unsigned long long, int> &b) { return a.first < b.first; });
        Tree t;
        for (size_t i = 0; i < order.size(); ++i) {
            if (i + 1 < order.size() && order[i + 1].first == order[i].first) continue;
            t.keys.push_back(order[i].first); t.rows.push_back(gyro + (size_t)order[i].second * 4); t.has.push_back(gyro_has ? gyro_has[order[i].second] : 1);
        }
        const double *e = est + (size_t)est_first[r] * 4;
        const uint8_t *eh = est_has ? est_has + est_first[r] : nullptr;
        const int n = est_first[r + 1] - est_first[r];
        bool any = false;
        double low_offs = 0.0, low = 0.0;
        for (size_t i = 0; i < steps; ++i) {
            const double offs = initial_offset - search_size + (double)i, c = cost_of(offs, e, eh, n, t);
            if (!any || !(low < c)) { low = c; low_offs = offs; any = true; }
        }
        if (!any) continue;
        results[r * 4] = low_offs; results[r * 4 + 1] = low;
        const double step = 2.0 / 200.0;
        double fine_offs = 0.0, fine = 0.0;
        for (int i = 0; i < 200; ++i) {
            const double offs = low_offs + (-2.0 + ((double)i * step)), c = cost_of(offs, e, eh, n, t);
            if (i == 0 || !(fine < c)) { fine = c; fine_offs = offs; }
        }
        results[r * 4 + 2] = fine_offs; results[r * 4 + 3] = fine;
    }
}
