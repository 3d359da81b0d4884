// test_flow_host.cpp — TEST INFRASTRUCTURE: gfw_flow_pyrlk's host code (gfw_flow_host.h: the check, the level sizes, the grid, the plan, the staging) in a program of
// its own, built with AddressSanitizer and UBSan (tests/test_cpp_flow_host.py; host pass only, no device, no library).  The packer fills a heap block of EXACTLY
// its plan's total — one byte more is the sanitizer's — at a fake device base; the caller's arrays are heap blocks of exactly their sizes too, so a check or a
// fill that reads or writes past them shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_flow.h"
#include "../../gyroflow_amd/csrc/gfw_flow_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static char *const D = (char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced
static const uint8_t *const PYR = (const uint8_t *)(uintptr_t)0x600000000000ull;

struct Call {
    int w = 200, h = 168, stride = 208, mode = 0, reserved = 0, on_device = 0;
    std::vector<uint8_t> frames;
    std::vector<int32_t> pairs, first;
    std::vector<float> feats;
    GfwFlowInputs inputs() const {
        return GfwFlowInputs{w, h, stride, mode, reserved, frames.data(), on_device, (int)first.size() - 1, pairs.data(), (int)pairs.size() / 2, first.data(), feats.data()};
    }
};
static Call make_call(const std::vector<int> &counts, const std::vector<int> &pairs) {
    Call c;
    c.first.push_back(0);
    for (int n : counts) c.first.push_back(c.first.back() + n);
    c.feats.resize((size_t)c.first.back() * 2);
    for (size_t i = 0; i < c.feats.size(); ++i) c.feats[i] = (float)i * 0.25f;
    c.frames.resize(counts.size() * (size_t)c.stride * c.h);
    for (size_t i = 0; i < c.frames.size(); ++i) c.frames[i] = (uint8_t)(i * 7);
    c.pairs.assign(pairs.begin(), pairs.end());
    return c;
}
static bool refused(const GfwFlowInputs &I, const char *text) {
    char why[256] = "";
    const bool ok = gfw_flow_check(I, why, sizeof(why));
    if (ok || !strstr(why, text)) { fprintf(stderr, "expected a refusal with \"%s\", got %s \"%s\"\n", text, ok ? "acceptance" : "", why); return false; }
    return true;
}

static void test_levels_and_grid() {
    int lw[4], lh[4];
    CHECK(gfw_flow_levels(200, 168, lw, lh) == 2 && lw[1] == 100 && lh[1] == 84 && lw[2] == 50 && lh[2] == 42 && lw[3] == 25 && lh[3] == 21);      // the cut: 21 < 24
    CHECK(gfw_flow_levels(384, 216, lw, lh) == 3 && lw[3] == 48 && lh[3] == 27);
    CHECK(gfw_flow_levels(24, 24, lw, lh) == 0);
    CHECK(gfw_flow_levels(47, 8192, lw, lh) == 1 && lw[1] == 24 && lh[1] == 4096);
    CHECK(gfw_flow_levels(8192, 8192, lw, lh) == 3 && lw[3] == 1024);
    CHECK(gfw_flow_levels(185, 185, lw, lh) == 3 && lw[3] == 24);
    CHECK(gfw_flow_levels(184, 185, lw, lh) == 2);
    GfwFlowGrid g = gfw_flow_grid(200, 168);
    CHECK(g.step == 13 && g.half == 5 && g.cols == 16 && g.rows == 13 && g.nodes == 208);
    g = gfw_flow_grid(1280, 720);
    CHECK(g.step == 85 && g.half == 13 && g.cols == 16 && g.rows == 9);              // round(25.6) = 26
    g = gfw_flow_grid(24, 8192);
    CHECK(g.step == 1 && g.nodes == 24 * 8192);
    g = gfw_flow_grid(8192, 24);
    CHECK(g.step == 546 && g.half == 82 && g.cols == 16 && g.rows == 1);
}

static void test_check() {
    Call c = make_call({70, 3, 0}, {0, 1, 1, 2, 0, 2});
    char why[256] = "";
    CHECK(gfw_flow_check(c.inputs(), why, sizeof(why)));
    { Call x = c; x.reserved = 1; CHECK(refused(x.inputs(), "reserved")); }
    { Call x = c; x.w = 23; CHECK(refused(x.inputs(), "frames of 23 x 168")); }
    { Call x = c; x.h = 8193; CHECK(refused(x.inputs(), "frames of 200 x 8193")); }
    { Call x = c; x.stride = 199; CHECK(refused(x.inputs(), "stride 199 under the width 200")); }
    { Call x = c; x.mode = 2; CHECK(refused(x.inputs(), "point mode 2")); }
    { GfwFlowInputs I = c.inputs(); I.n_pairs = -1; CHECK(refused(I, "negative count")); }
    { GfwFlowInputs I = c.inputs(); I.n_frames = -1; CHECK(refused(I, "negative count")); }
    { GfwFlowInputs I = c.inputs(); I.n_frames = GFW_FLOW_FRAMES_MAX + 1; CHECK(refused(I, "4097 frames")); }
    { GfwFlowInputs I = c.inputs(); I.n_pairs = GFW_FLOW_PAIRS_MAX + 1; CHECK(refused(I, "65536 pairs")); }
    { GfwFlowInputs I = c.inputs(); I.pair_frames = nullptr; CHECK(refused(I, "without pair_frames")); }
    { GfwFlowInputs I = c.inputs(); I.frames = nullptr; CHECK(refused(I, "without their planes")); }
    { GfwFlowInputs I = c.inputs(); I.feat_first = nullptr; CHECK(refused(I, "point mode 0 without features")); }
    { GfwFlowInputs I = c.inputs(); I.features = nullptr; CHECK(refused(I, "point mode 0 without features")); }
    { Call x = c; x.first = {0, 70, 60, 73}; CHECK(refused(x.inputs(), "frame 1: feat_first descends (60 after 70)")); }
    { Call x = c; x.first = {-1, 70, 73, 73}; CHECK(refused(x.inputs(), "frame 0: feat_first -1 is negative")); }
    { Call x = c; x.first = {0, 70, 73, 73 + 4097}; CHECK(refused(x.inputs(), "frame 2: 4097 features")); }
    { Call x = c; x.pairs[3] = 3; CHECK(refused(x.inputs(), "pair 1: frames (1, 3) outside the call's 3 frames")); }
    { Call x = c; x.pairs[4] = -1; CHECK(refused(x.inputs(), "pair 2: frames (-1, 2) outside")); }
    { Call x = c; x.pairs[5] = 0; CHECK(refused(x.inputs(), "pair 2: frame 0 paired with itself")); }
    { Call x = c; x.mode = 1; x.w = 24; x.stride = 24; x.h = 8192; CHECK(refused(x.inputs(), "has 196608 nodes")); }
    // the 2 GiB of one staged block: host frames of a huge stride are refused without being read (the vector holds three small frames); device frames are not staged
    { Call x = c; x.stride = 1 << 20; x.h = 8192; CHECK(refused(x.inputs(), "at most 2 GiB")); }
    { Call x = c; x.stride = 1 << 20; x.h = 8192; x.on_device = 1; CHECK(gfw_flow_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.stride = (1 << 20) / 3; x.h = 2048; CHECK(gfw_flow_check(x.inputs(), why, sizeof(why)) && gfw_flow_plan(x.inputs()).total < GFW_FLOW_STAGED_MAX); }
    // no pairs: accepted whatever else is null; the grid mode needs no features
    { GfwFlowInputs I = c.inputs(); I.n_pairs = 0; I.pair_frames = nullptr; I.frames = nullptr; I.feat_first = nullptr; CHECK(gfw_flow_check(I, why, sizeof(why))); }
    { GfwFlowInputs I = c.inputs(); I.mode = 1; I.feat_first = nullptr; I.features = nullptr; CHECK(gfw_flow_check(I, why, sizeof(why))); }
}

static void stage(const Call &c) {
    const GfwFlowInputs I = c.inputs();
    char why[256] = "";
    CHECK(gfw_flow_check(I, why, sizeof(why)));
    const GfwFlowPlan P = gfw_flow_plan(I);
    char *block = (char *)malloc(P.total ? P.total : 1);
    memset(block, 0xEE, P.total);
    GfwFlowArgs A;
    memset(&A, 0, sizeof(A));
    gfw_flow_fill(P, I, block, D, PYR, A);
    const int n_pairs = I.n_pairs, n_frames = I.n_frames;
    const int32_t *raw = (const int32_t *)(block + P.o_raw);
    CHECK(memcmp(block + P.o_pairs, c.pairs.data(), sizeof(int32_t) * c.pairs.size()) == 0);
    CHECK(raw[0] == 0 && raw[n_pairs] == (int32_t)P.raw_total);
    int most = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int a = c.pairs[(size_t)p * 2], n = c.mode ? P.grid.nodes : c.first[(size_t)a + 1] - c.first[(size_t)a];
        CHECK(raw[p + 1] - raw[p] == n);
        if (n > most) most = n;
    }
    CHECK(A.max_features == most && A.n_pairs == n_pairs && A.n_frames == n_frames && A.mode == c.mode && A.top == P.top);
    CHECK((const char *)A.pair_frames == D + P.o_pairs && (const char *)A.raw_first == D + P.o_raw && (char *)A.kept == D + P.o_kept);
    for (int p = 0; p < n_pairs; ++p) CHECK(((const int32_t *)(block + P.o_kept))[p] == 0);
    if (c.mode == 0) {
        const int32_t *ff = (const int32_t *)(block + P.o_ffirst);
        for (int f = 0; f <= n_frames; ++f) CHECK(ff[f] == c.first[(size_t)f] - c.first[0]);
        CHECK(!P.n_features || memcmp(block + P.o_feat, c.feats.data() + (size_t)c.first[0] * 2, sizeof(float) * 2 * (size_t)P.n_features) == 0);
        CHECK((const char *)A.feat_first == D + P.o_ffirst && (const char *)A.features == D + P.o_feat);
    } else CHECK(!A.feat_first && !A.features && A.grid_nodes == P.grid.nodes && A.grid_rows == P.grid.rows && A.grid_step == P.grid.step && A.grid_half == P.grid.half);
    if (c.on_device) CHECK(A.lv[0].base == c.frames.data() && P.o_frames + 0 == P.total);
    else { CHECK((const char *)A.lv[0].base == D + P.o_frames && memcmp(block + P.o_frames, c.frames.data(), c.frames.size()) == 0 && P.total >= P.o_frames + c.frames.size()); }
    CHECK(A.lv[0].w == c.w && A.lv[0].h == c.h && A.lv[0].stride == c.stride && A.lv[0].frame_bytes == (int64_t)c.stride * c.h);
    size_t at = 0;
    for (int l = 1; l < GFW_FLOW_LEVELS; ++l) {
        if (l > P.top) { CHECK(!A.lv[l].base && A.lv[l].w == 0); continue; }
        CHECK(A.lv[l].base == PYR + P.level_at[l] && P.level_at[l] >= at && P.level_at[l] % 8 == 0);
        CHECK(A.lv[l].w == P.lw[l] && A.lv[l].stride == P.lw[l] && A.lv[l].frame_bytes == (int64_t)P.lw[l] * P.lh[l]);
        at = P.level_at[l] + (size_t)n_frames * P.lw[l] * P.lh[l];
    }
    CHECK(P.pyramid_bytes >= at);
    free(block);
}

static void test_staging() {
    Call c = make_call({70, 3, 0}, {0, 1, 1, 2, 0, 2, 2, 0});
    stage(c);
    { Call x = c; x.on_device = 1; stage(x); }
    { Call x = c; x.mode = 1; stage(x); }
    { Call x = c; x.first = {5, 75, 78, 78}; x.feats.resize(78 * 2, 1.0f); stage(x); }                 // a feat_first that does not start at 0
    { Call x = make_call({0, 0}, {0, 1}); stage(x); }                                                   // pairs without features
    { Call x = make_call({4, 4}, {1, 0}); x.w = 24; x.h = 24; x.stride = 24; x.frames.resize(2 * 24 * 24); stage(x); }      // one level
}

int main() {
    test_levels_and_grid();
    test_check();
    test_staging();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("flow host code ok\n");
    return 0;
}
