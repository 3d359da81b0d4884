// gfw_pairs_host.h — host only: what the calls over frame pairs with matched points (gfw_sync_visual_*, gfw_pose_almeida, gfw_pose_essential, gfw_sync_rs_*) share
// on the host — the check of the pair set, the staging of its firsts and points, and the gate on the lens the kernel parameters describe.  The calls' own packers
// (gfw_sync_host.h, gfw_pose_host.h, gfw_pose_essential_host.h, gfw_sync_rs_host.h) include it behind include/gfwarp.h; no kernel's translation unit sees it, it calls nothing of HIP.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "gfw_layout.h"

// The frame pairs of a call: pair p's points are entries pair_first[p] .. pair_first[p + 1] of points_a / points_b ([..][2] f32); pair_ts_us [n_pairs][2], null
// where the call takes no timestamps
struct GfwPairSet { const int64_t *pair_ts_us; const int32_t *pair_first; const float *points_a, *points_b; int n_pairs; };
// What differs between the calls: the noun of the "bad .. arguments" texts, the most pairs of a call and points of a pair, whether pair_ts_us is required, and whether
// the points count from pair_first[0] (staged: firsts from 0, the points from that entry on) or from 0 (staged: pair_first as given, the points from the arrays' start)
struct GfwPairRules { const char *noun; int pairs_max, pair_max; bool needs_ts, from_first; };

// the points a call stages
inline int gfw_pairs_total(const GfwPairSet &P, bool from_first) { return P.n_pairs ? P.pair_first[P.n_pairs] - (from_first ? P.pair_first[0] : 0) : 0; }
// -> true with the points the call stages and those of its largest pair, or false with the reason (the pair named) in `err`
inline bool gfw_pairs_check(const GfwPairSet &P, const GfwPairRules &R, int &total, int &max_pair, char *err, size_t cap) {
    total = max_pair = 0;
    if (P.n_pairs < 0 || P.n_pairs > R.pairs_max) { snprintf(err, cap, "%d pairs: at most %d in a call", P.n_pairs, R.pairs_max); return false; }
    if (P.n_pairs == 0) return true;
    if (!P.pair_first || (R.needs_ts && !P.pair_ts_us)) { snprintf(err, cap, "bad %s arguments (pairs without pair_first%s)", R.noun, R.needs_ts ? " / pair_ts_us" : ""); return false; }
    if (P.pair_first[0] < 0) { snprintf(err, cap, "pair 0: pair_first %d is negative", P.pair_first[0]); return false; }
    for (int p = 0; p < P.n_pairs; ++p) {
        if (P.pair_first[p + 1] < P.pair_first[p]) { snprintf(err, cap, "pair %d: pair_first descends (%d after %d)", p, P.pair_first[p + 1], P.pair_first[p]); return false; }
        const int n = P.pair_first[p + 1] - P.pair_first[p];
        if (n > R.pair_max) { snprintf(err, cap, "pair %d: %d points, at most %d", p, n, R.pair_max); return false; }
        if (n > max_pair) max_pair = n;
    }
    total = gfw_pairs_total(P, R.from_first);
    if (total && (!P.points_a || !P.points_b)) { snprintf(err, cap, "bad %s arguments (%d points without points_a / points_b)", R.noun, total); return false; }
    return true;
}

// The staged parts: [n_pairs + 1] first points, then the `total` points of the first frames and those of the second, added to a layout -> their offsets.  Where a
// call keeps a part of its own between the two it adds them itself
inline void gfw_pairs_add(BlockLayout &L, int n_pairs, size_t total, size_t &o_first, size_t &o_pts) {
    o_first = L.add(sizeof(int32_t) * ((size_t)n_pairs + 1)); o_pts = L.add(sizeof(float) * 2 * total * 2);
}
// Fills them at (h, d) -> the points staged, and the device pointers of the two parts
inline int gfw_pairs_fill(size_t o_first, size_t o_pts, const GfwPairSet &P, bool from_first, char *h, const char *d, const int32_t *&d_first, const float *&d_points) {
    int32_t *first = (int32_t *)(h + o_first);
    const int32_t base = P.n_pairs && from_first ? P.pair_first[0] : 0;
    const int total = gfw_pairs_total(P, from_first);
    if (base) for (int p = 0; p <= P.n_pairs; ++p) first[p] = P.pair_first[p] - base;
    else if (P.n_pairs) memcpy(first, P.pair_first, sizeof(int32_t) * ((size_t)P.n_pairs + 1));
    else first[0] = 0;
    const size_t pb = sizeof(float) * 2 * (size_t)total;
    if (total) { memcpy(h + o_pts, P.points_a + (size_t)base * 2, pb); memcpy(h + o_pts + pb, P.points_b + (size_t)base * 2, pb); }
    d_first = (const int32_t *)(d + o_first); d_points = (const float *)(d + o_pts);
    return total;
}

// The lens these calls cover, of the kernel parameters `p`.  `what`: the call's phrase in front of "does not cover"
inline bool gfw_pairs_lens_flags(int flags, const char *what, char *err, size_t cap) {
    if (!(flags & (256 | 512 | 1024))) return true;                          // HAS_IBIS_DATA | HAS_MESH_DATA | HAS_FPD_DATA
    snprintf(err, cap, "%s does not cover per-frame IBIS/OIS shifts, lens meshes or focal-plane distortion data (flags 0x%x)", what, flags); return false;
}
struct GfwPairSizes { int video_w, video_h, flow_w, flow_h; };
// -> true, or false with the reason in `err`: a video or optical-flow size under 1 or `own_ok` false (the configuration's text ends with the call's own fields,
// `own_fmt` ..), the flags, or f / c that are not the f32 cast of the camera matrix K
__attribute__((format(printf, 9, 10)))
inline bool gfw_pairs_lens_check(const gfw_kernel_params &p, const double *K, const GfwPairSizes &Z, const char *noun, const char *what, bool own_ok, char *err, size_t cap, const char *own_fmt, ...) {
    if (Z.video_w < 1 || Z.video_h < 1 || Z.flow_w < 1 || Z.flow_h < 1 || !own_ok) {
        const int at = snprintf(err, cap, "bad %s configuration: video %d x %d, optical flow %d x %d, ", noun, Z.video_w, Z.video_h, Z.flow_w, Z.flow_h);
        va_list ap; va_start(ap, own_fmt);
        if (at >= 0 && (size_t)at < cap) vsnprintf(err + at, cap - (size_t)at, own_fmt, ap);
        va_end(ap); return false; }
    if (!gfw_pairs_lens_flags(p.flags, what, err, cap)) return false;
    if (p.f[0] != (float)K[0] || p.f[1] != (float)K[4] || p.c[0] != (float)K[2] || p.c[1] != (float)K[5]) {
        snprintf(err, cap, "the kernel parameters' f (%g, %g) / c (%g, %g) are not the f32 cast of camera_matrix (%g, %g) / (%g, %g)", (double)p.f[0], (double)p.f[1], (double)p.c[0], (double)p.c[1], K[0], K[4], K[2], K[5]);
        return false; }
    return true;
}
