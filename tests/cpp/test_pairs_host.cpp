// test_pairs_host.cpp — TEST INFRASTRUCTURE: the host code the point-pair calls share (gfw_pairs_host.h: the pair-set check, the staged firsts and points, the lens
// gate) and the visual search's check (gfw_sync_host.h: gfw_sync_check) in a program of their own, built with AddressSanitizer and UBSan
// (tests/test_cpp_pairs_host.py; host pass only, no device, no library).  The packer fills a heap block of EXACTLY its layout's total — one byte more is the
// sanitizer's — at a fake device base; the caller's arrays are heap blocks of exactly their sizes too, so a check or a fill that reads or writes past them shows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_sync.h"
#include "../../gyroflow_amd/csrc/gfw_sync_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static const char *const D = (const char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced

// made-up limits: 3 pairs a call, 5 points a pair
static GfwPairRules rules(bool needs_ts, bool from_first) { return GfwPairRules{"toy", 3, 5, needs_ts, from_first}; }
struct Pairs {
    std::vector<int64_t> ts; std::vector<int32_t> first; std::vector<float> a, b;
    GfwPairSet set() const { return GfwPairSet{ts.data(), first.data(), a.data(), b.data(), (int)first.size() - 1}; }
};
// pairs of `sizes` points behind `lead` unused ones; a's entries count from 0, b's from 1000
static Pairs make_pairs(std::initializer_list<int> sizes, int lead) {
    Pairs p;
    p.first.push_back(lead);
    for (int n : sizes) { p.first.push_back(p.first.back() + n); p.ts.push_back(1000 * (int64_t)p.first.size()); p.ts.push_back(1000 * (int64_t)p.first.size() + 500); }
    p.a.resize((size_t)p.first.back() * 2); p.b.resize(p.a.size());
    for (size_t i = 0; i < p.a.size(); ++i) { p.a[i] = (float)i; p.b[i] = 1000.0f + (float)i; }
    return p;
}
static bool refused(const GfwPairSet &P, const GfwPairRules &R, const char *text) {
    char why[256] = "";
    int total, max_pair;
    const bool ok = gfw_pairs_check(P, R, total, max_pair, why, sizeof(why));
    if (ok || strcmp(why, text)) fprintf(stderr, "expected the refusal '%s', got %s '%s'\n", text, ok ? "acceptance" : "refusal", why);
    return !ok && !strcmp(why, text);
}

static void test_check() {
    char why[256];
    int total, max_pair;
    for (int from_first = 0; from_first < 2; ++from_first) {
        const GfwPairRules R = rules(true, from_first != 0), R_no_ts = rules(false, from_first != 0);
        const GfwPairSet none = {nullptr, nullptr, nullptr, nullptr, 0};
        total = max_pair = 7;
        CHECK(gfw_pairs_check(none, R, total, max_pair, why, sizeof(why)) && total == 0 && max_pair == 0);
        { GfwPairSet P = none; P.n_pairs = -1; CHECK(refused(P, R, "-1 pairs: at most 3 in a call")); }
        { const Pairs p = make_pairs({0, 1, 5}, 0); CHECK(gfw_pairs_check(p.set(), R, total, max_pair, why, sizeof(why)) && total == 6 && max_pair == 5); }      // sizes 0, 1, limit; n_pairs at its limit
        { const Pairs p = make_pairs({0, 6, 1}, 0); CHECK(refused(p.set(), R, "pair 1: 6 points, at most 5")); }
        { const Pairs p = make_pairs({1, 1, 1, 1}, 0); CHECK(refused(p.set(), R, "4 pairs: at most 3 in a call")); }
        const Pairs p = make_pairs({2, 0, 3}, 2);
        { GfwPairSet P = p.set(); P.pair_first = nullptr; CHECK(refused(P, R, "bad toy arguments (pairs without pair_first / pair_ts_us)") && refused(P, R_no_ts, "bad toy arguments (pairs without pair_first)")); }
        { GfwPairSet P = p.set(); P.pair_ts_us = nullptr; CHECK(refused(P, R, "bad toy arguments (pairs without pair_first / pair_ts_us)")); CHECK(gfw_pairs_check(P, R_no_ts, total, max_pair, why, sizeof(why))); }
        { Pairs x = make_pairs({0, 0}, 4); x.a.clear(); x.b.clear(); GfwPairSet P = x.set(); P.points_a = P.points_b = nullptr;                // no points staged: none needed
          CHECK((from_first ? gfw_pairs_check(P, R, total, max_pair, why, sizeof(why)) && total == 0 : refused(P, R, "bad toy arguments (4 points without points_a / points_b)"))); }
        { Pairs x = make_pairs({0, 0}, 0); GfwPairSet P = x.set(); P.points_a = P.points_b = nullptr; CHECK(gfw_pairs_check(P, R, total, max_pair, why, sizeof(why)) && total == 0); }
        { Pairs x = make_pairs({0, 1}, 0); GfwPairSet P = x.set(); P.points_a = nullptr; CHECK(refused(P, R, "bad toy arguments (1 points without points_a / points_b)")); }
        { Pairs x = make_pairs({0, 1}, 0); GfwPairSet P = x.set(); P.points_b = nullptr; CHECK(refused(P, R, "bad toy arguments (1 points without points_a / points_b)")); }
        { Pairs x = p; x.first[0] = -1; CHECK(refused(x.set(), R, "pair 0: pair_first -1 is negative")); }
        { Pairs x = p; x.first[3] = 3; CHECK(refused(x.set(), R, "pair 2: pair_first descends (3 after 4)")); }                             // a descent at the last pair
        char tiny[8];
        { Pairs x = p; x.first[3] = 3; GfwPairSet P = x.set(); CHECK(!gfw_pairs_check(P, R, total, max_pair, tiny, sizeof(tiny)) && !strcmp(tiny, "pair 2:")); }      // cut to the caller's room
    }
}

static void test_fill() {
    for (int from_first = 0; from_first < 2; ++from_first) {
        Pairs p = make_pairs({0, 4, 5}, 3);                                   // pair_first = {3, 3, 7, 12}
        const GfwPairSet P = p.set();
        char why[256];
        int total, max_pair;
        CHECK(gfw_pairs_check(P, rules(false, from_first != 0), total, max_pair, why, sizeof(why)));
        CHECK(total == (from_first ? 9 : 12) && max_pair == 5 && gfw_pairs_total(P, from_first != 0) == total);
        BlockLayout L;
        const size_t o_own = L.add(5);                                        // a part of the call's own in front: the shared parts start behind it, on a multiple of 8
        size_t o_first = 0, o_pts = 0;
        gfw_pairs_add(L, P.n_pairs, (size_t)total, o_first, o_pts);
        CHECK(o_own == 0 && o_first == 8 && o_pts == 8 + 16 && L.total == 8 + 16 + 16 * (size_t)total);
        char *h = (char *)malloc(L.total);                                    // exactly the layout's bytes
        memset(h, 0xA5, L.total);
        const int32_t *d_first = nullptr; const float *d_points = nullptr;
        CHECK(gfw_pairs_fill(o_first, o_pts, P, from_first != 0, h, D, d_first, d_points) == total);
        CHECK((const char *)d_first == D + o_first && (const char *)d_points == D + o_pts);
        const int32_t rebased[4] = {0, 0, 4, 9};
        CHECK(!memcmp(h + o_first, from_first ? rebased : p.first.data(), 16));
        const size_t skip = from_first ? 3 : 0, pb = 8 * (size_t)total;
        CHECK(!memcmp(h + o_pts, p.a.data() + skip * 2, pb) && !memcmp(h + o_pts + pb, p.b.data() + skip * 2, pb));
        CHECK((unsigned char)h[5] == 0xA5);                                   // the part in front is not the packer's
        free(h);
    }
    // no pairs: one first, 0
    BlockLayout L;
    size_t o_first = 7, o_pts = 7;
    gfw_pairs_add(L, 0, 0, o_first, o_pts);
    CHECK(L.total == 8 && o_first == 0 && o_pts == 8);
    char *h = (char *)malloc(L.total);
    const int32_t *d_first = nullptr; const float *d_points = nullptr;
    CHECK(gfw_pairs_fill(o_first, o_pts, GfwPairSet{nullptr, nullptr, nullptr, nullptr, 0}, true, h, D, d_first, d_points) == 0 && *(int32_t *)h == 0 && (const char *)d_first == D);
    free(h);
}

static bool lens_check(const gfw_kernel_params &p, const double *K, const int *sizes, bool own_ok, char *why, size_t cap) {
    return gfw_pairs_lens_check(p, K, {sizes[0], sizes[1], sizes[2], sizes[3]}, "toy", "the toy search", own_ok, why, cap, "gain %g, taps %d", 2.5, 7);
}
static void test_lens() {
    const double K[9] = {1000.1, 0.0, 959.3, 0.0, 1001.7, 539.9, 0.0, 0.0, 1.0};
    const int sizes[4] = {1920, 1080, 960, 540};
    gfw_kernel_params good;
    memset(&good, 0, sizeof(good));
    good.f[0] = (float)K[0]; good.f[1] = (float)K[4]; good.c[0] = (float)K[2]; good.c[1] = (float)K[5];
    char why[256];
    CHECK(lens_check(good, K, sizes, true, why, sizeof(why)));
    CHECK(!lens_check(good, K, sizes, false, why, sizeof(why)) && !strcmp(why, "bad toy configuration: video 1920 x 1080, optical flow 960 x 540, gain 2.5, taps 7"));
    for (int bit : {256, 512, 1024}) {
        gfw_kernel_params p = good; p.flags = bit | 3;
        char want[256];
        snprintf(want, sizeof(want), "the toy search does not cover per-frame IBIS/OIS shifts, lens meshes or focal-plane distortion data (flags 0x%x)", bit | 3);
        CHECK(!lens_check(p, K, sizes, true, why, sizeof(why)) && !strcmp(why, want));
        CHECK(!gfw_pairs_lens_flags(bit, "the toy search", why, sizeof(why)) && strstr(why, "the toy search does not cover"));
    }
    { gfw_kernel_params p = good; p.flags = 255 | 2048; CHECK(lens_check(p, K, sizes, true, why, sizeof(why))); }      // other bits pass
    for (int k = 0; k < 4; ++k)
        for (float to : {-INFINITY, INFINITY}) {                             // one f32 step to either side of the cast
            gfw_kernel_params p = good;
            float &v = k < 2 ? p.f[k] : p.c[k - 2];
            v = nextafterf(v, to);
            CHECK(!lens_check(p, K, sizes, true, why, sizeof(why)) && strstr(why, "are not the f32 cast of camera_matrix"));
        }
    for (int k = 0; k < 4; ++k) {
        int s[4] = {sizes[0], sizes[1], sizes[2], sizes[3]};
        s[k] = 0;
        CHECK(!lens_check(good, K, s, true, why, sizeof(why)) && strstr(why, "bad toy configuration: video ") && strstr(why, ", gain 2.5, taps 7"));
    }
    char tiny[8];
    { const int s[4] = {1920, 1080, 960, 0}; CHECK(!lens_check(good, K, s, true, tiny, sizeof(tiny)) && !strcmp(tiny, "bad toy")); }
}

static gfw_sync_search make_search(int w, int h) {
    gfw_sync_search s;
    memset(&s, 0, sizeof(s));
    s.width = w; s.height = h; s.use_sync_offsets = 1;
    return s;
}
struct SyncCheck { bool ok; int total, max_pair, n_coarse; char why[256]; };
static SyncCheck sync_check(const gfw_sync_search *s, int flags, const GfwPairSet &P, const double *cand, int n_cand, int mode, double size_ms, double fps, const void *out) {
    SyncCheck r;
    memset(&r, 0, sizeof(r));
    r.ok = gfw_sync_check(s, flags, P, cand, n_cand, mode, size_ms, fps, out, r.total, r.max_pair, r.n_coarse, r.why, sizeof(r.why));
    return r;
}
static void test_sync_check() {
    const Pairs p = make_pairs({4, 0, 4}, 0);
    const GfwPairSet P = p.set();
    const double cand[6] = {0.0, 1.0, 2.0, 3.0, 4.0, 5.0};
    double costs[3];
    gfw_sync_result result;
    const gfw_sync_search s = make_search(1920, 1080);
    { const SyncCheck r = sync_check(&s, 0, P, cand, 3, -1, 0, 0, costs); CHECK(r.ok && r.total == 8 && r.max_pair == 4 && r.n_coarse == 3); }
    CHECK(!sync_check(nullptr, 0, P, cand, 3, -1, 0, 0, costs).ok);
    { const gfw_sync_search big = make_search(46340, 46340); CHECK(sync_check(&big, 0, P, cand, 3, -1, 0, 0, costs).ok); }
    { const gfw_sync_search big = make_search(46341, 46341); const SyncCheck r = sync_check(&big, 0, P, cand, 3, -1, 0, 0, costs); CHECK(!r.ok && strstr(r.why, "must stay below 2^32")); }
    { gfw_sync_search x = s; x.horizontal_readout = 2; const SyncCheck r = sync_check(&x, 0, P, cand, 3, -1, 0, 0, costs); CHECK(!r.ok && strstr(r.why, "horizontal_readout 2")); }
    { gfw_sync_search x = s; x.reserved[1] = 1; const SyncCheck r = sync_check(&x, 0, P, cand, 3, -1, 0, 0, costs); CHECK(!r.ok && strstr(r.why, "reserved slots must be 0")); }
    { const SyncCheck r = sync_check(&s, 512, P, cand, 3, -1, 0, 0, costs); CHECK(!r.ok && strstr(r.why, "the sync search does not cover")); }
    { const SyncCheck r = sync_check(&s, 0, P, nullptr, 0, 2, 5.0, 30.0, &result); CHECK(!r.ok && !strcmp(r.why, "bad sync arguments (mode 2, or a null result)")); }
    { const SyncCheck r = sync_check(&s, 0, P, nullptr, 0, 0, 5.0, 30.0, nullptr); CHECK(!r.ok && strstr(r.why, "a null result")); }
    { const SyncCheck r = sync_check(&s, 0, P, nullptr, 0, 0, 1000001.0, 30.0, &result); CHECK(!r.ok && strstr(r.why, "a search of 1e+06 candidates")); }
    { const SyncCheck r = sync_check(&s, 0, P, nullptr, 0, 0, 1000000.0, 30.0, &result); CHECK(r.ok && r.n_coarse == 1000000); }
    { const SyncCheck r = sync_check(&s, 0, P, nullptr, 0, 1, 0.0, 30.0, &result); CHECK(r.ok && r.n_coarse == 66); }
    { const SyncCheck r = sync_check(&s, 0, P, nullptr, 3, -1, 0, 0, costs); CHECK(!r.ok && !strcmp(r.why, "bad sync arguments (candidates without their array / costs)")); }
    { const SyncCheck r = sync_check(&s, 0, P, cand, 3, -1, 0, 0, nullptr); CHECK(!r.ok && strstr(r.why, "candidates without their array / costs")); }
    CHECK(sync_check(&s, 0, P, nullptr, 0, -1, 0, 0, nullptr).ok);            // no candidates: nothing of theirs is needed
    { GfwPairSet x = P; x.pair_ts_us = nullptr; const SyncCheck r = sync_check(&s, 0, x, cand, 3, -1, 0, 0, costs); CHECK(!r.ok && !strcmp(r.why, "bad sync arguments (pairs without pair_first / pair_ts_us)")); }
    { Pairs x = make_pairs({GFW_SYNC_PAIR_MAX + 1}, 0); const SyncCheck r = sync_check(&s, 0, x.set(), cand, 3, -1, 0, 0, costs); CHECK(!r.ok && !strcmp(r.why, "pair 0: 4097 points, at most 4096")); }
    { const SyncCheck r = sync_check(&s, 0, P, cand, -1, -1, 0, 0, costs); CHECK(!r.ok && strstr(r.why, "a negative count")); }
}

int main() {
    test_check();
    test_fill();
    test_lens();
    test_sync_check();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("pairs host code ok\n");
    return 0;
}
