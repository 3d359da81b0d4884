// gfw_sync_gyro_host.h — host only: what gfw_sync_gyro_costs / gfw_sync_gyro_search stage for the kernels of gfw_sync_gyro.hip.  Included behind gfw_sync_gyro.h
// (GfwGyroRange, gfw_gyro_key) by gfw_api.hip, and by whatever else stages a call for those kernels; the kernels' translation unit does not see it.
#pragma once
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "gfw_layout.h"

// The staged block: [n_ranges] GfwGyroRange, the estimated samples [][4] f64 and their has bytes, the gyro keys and values [][4] f64, the candidates.
struct GfwGyroLayout { size_t o_ranges, o_est, o_has, o_keys, o_val, o_cand, total; };
inline GfwGyroLayout gfw_gyro_layout(int n_ranges, size_t tot_est, size_t tot_gyro, size_t tot_cand) {
    BlockLayout L;
    GfwGyroLayout G;
    G.o_ranges = L.add(sizeof(GfwGyroRange) * (size_t)n_ranges); G.o_est = L.add(32 * tot_est); G.o_has = L.add(tot_est);
    G.o_keys = L.add(8 * tot_gyro); G.o_val = L.add(32 * tot_gyro); G.o_cand = L.add(8 * tot_cand);
    G.total = L.total;
    return G;
}

// Host: what a call stages, filled into the caller's arrays (gfw_gyro_fill below: the parts of ONE block).  A series is the ABI's: range r owns first[r] .. first[r + 1] - 1 of data [][4] f64 (timestamp_ms, x, y, z)
// and of has (nullptr = all present).  Each range's gyro slice becomes the BTreeMap<usize, TimeIMU> of :50 flattened: keys ascending, a later sample with the same key
// replacing an earlier one — the slice need not be ascending.  Candidates: `n_coarse` of them per range made by :59 (cand_first nullptr), or the caller's.
// The arrays hold what the firsts span (keys / values: at most that) and are filled from 0 whatever first[0] is: ranges[r] holds offsets into the STAGED arrays, so
// costs laid out as the staged candidates start at the caller's entry cand_first[0].  -> the largest candidate count of a range.
struct GfwGyroSeries { const int32_t *first; const double *data; const uint8_t *has; };
inline int gfw_gyro_stage(const GfwGyroSeries &est, const GfwGyroSeries &gyro, int n_ranges, const int32_t *cand_first, const double *candidates, size_t n_coarse,
                          double initial_offset_ms, double search_size_ms, GfwGyroRange *ranges, double *h_est, uint8_t *h_has, unsigned long long *h_keys, double *h_val, double *h_cand) {
    typedef std::pair<unsigned long long, int> KeyAt;
    std::vector<KeyAt> order;
    size_t at_est = 0, at_gyro = 0, at_cand = 0;
    int max_cand = 0;
    for (int r = 0; r < n_ranges; ++r) {
        GfwGyroRange &G = ranges[r];
        const int e0 = est.first[r], en = est.first[r + 1] - e0, g0 = gyro.first[r], gn = gyro.first[r + 1] - g0;
        G.est_first = (long long)at_est; G.est_n = en; G.gyro_first = (long long)at_gyro; G.cand_first = (long long)at_cand; G.pad = 0;
        if (en) memcpy(h_est + at_est * 4, est.data + (size_t)e0 * 4, 32 * (size_t)en);
        for (int i = 0; i < en; ++i) h_has[at_est + i] = est.has ? (est.has[e0 + i] ? 1 : 0) : 1;
        at_est += (size_t)en;
        order.resize((size_t)gn);
        bool ascending = true;
        for (int i = 0; i < gn; ++i) {
            order[i] = KeyAt(gfw_gyro_key(gyro.data[(size_t)(g0 + i) * 4] * 1000.0), g0 + i);
            if (i && order[i].first <= order[i - 1].first) ascending = false;
        }
        if (!ascending) std::stable_sort(order.begin(), order.end(), [](const KeyAt &a, const KeyAt &b) { return a.first < b.first; });
        int kept = 0;
        for (int i = 0; i < gn; ++i) {
            if (i + 1 < gn && order[i + 1].first == order[i].first) continue;            // an equal key follows: that later sample wins
            const double *v = gyro.data + (size_t)order[i].second * 4;
            h_keys[at_gyro + kept] = order[i].first;
            double *o = h_val + (at_gyro + kept) * 4;
            o[0] = v[1]; o[1] = v[2]; o[2] = v[3]; o[3] = (!gyro.has || gyro.has[order[i].second]) ? 1.0 : 0.0;
            ++kept;
        }
        G.gyro_n = kept;
        at_gyro += (size_t)kept;
        if (!cand_first) {
            G.cand_n = (int)n_coarse;
            for (size_t i = 0; i < n_coarse; ++i) h_cand[at_cand + i] = initial_offset_ms - search_size_ms + (double)i;       // :59
        } else {
            G.cand_n = cand_first[r + 1] - cand_first[r];
            if (G.cand_n) memcpy(h_cand + at_cand, candidates + cand_first[r], 8 * (size_t)G.cand_n);
        }
        at_cand += (size_t)G.cand_n;
        if (G.cand_n > max_cand) max_cand = G.cand_n;
    }
    return max_cand;
}
// The same into the block at (h, d) — the layout above — with the argument block's input pointers.
inline int gfw_gyro_fill(const GfwGyroLayout &L, const GfwGyroSeries &est, const GfwGyroSeries &gyro, int n_ranges, const int32_t *cand_first, const double *candidates,
                         size_t n_coarse, double initial_offset_ms, double search_size_ms, char *h, const char *d, GfwGyroArgs &A) {
    A.ranges = (const GfwGyroRange *)(d + L.o_ranges); A.est = (const double *)(d + L.o_est); A.est_has = (const uint8_t *)(d + L.o_has);
    A.keys = (const unsigned long long *)(d + L.o_keys); A.gyro = (const double *)(d + L.o_val); A.candidates = (const double *)(d + L.o_cand);
    return gfw_gyro_stage(est, gyro, n_ranges, cand_first, candidates, n_coarse, initial_offset_ms, search_size_ms, (GfwGyroRange *)(h + L.o_ranges), (double *)(h + L.o_est),
                          (uint8_t *)(h + L.o_has), (unsigned long long *)(h + L.o_keys), (double *)(h + L.o_val), (double *)(h + L.o_cand));
}
