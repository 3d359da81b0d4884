// test_dis_host.cpp — TEST INFRASTRUCTURE: gfw_flow_dis's host code (gfw_dis_host.h: the check, the coarsest scale and the level sizes, the plan, the staging) in a
// program of its own, built with AddressSanitizer and UBSan (tests/test_cpp_dis_host.py; host pass only, no device, no library).  The packer fills a heap block of
// EXACTLY its plan's total — one byte more is the sanitizer's — at a fake device base; the caller's arrays are heap blocks of exactly their sizes too, so a check or
// a fill that reads or writes past them shows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_flow.h"
#include "../../gyroflow_amd/csrc/gfw_flow_host.h"
#include "../../gyroflow_amd/csrc/gfw_dis.h"
#include "../../gyroflow_amd/csrc/gfw_dis_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static char *const D = (char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced
static char *const WORK = (char *)(uintptr_t)0x600000000000ull;  // the device work space: never dereferenced

struct Call {
    int w = 200, h = 168, stride = 208, finest = 2, variational = 0, reserved = 0, on_device = 0, n_frames = 3;
    std::vector<uint8_t> frames;
    std::vector<int32_t> pairs;
    GfwDisInputs inputs() const { return GfwDisInputs{w, h, stride, finest, variational, reserved, frames.data(), on_device, n_frames, pairs.data(), (int)pairs.size() / 2}; }
};
static Call make_call(int n_frames, const std::vector<int> &pairs) {
    Call c;
    c.n_frames = n_frames;
    c.frames.resize((size_t)n_frames * c.stride * c.h);
    for (size_t i = 0; i < c.frames.size(); ++i) c.frames[i] = (uint8_t)(i * 7);
    c.pairs.assign(pairs.begin(), pairs.end());
    return c;
}
static bool refused(const GfwDisInputs &I, const char *text) {
    char why[256] = "";
    const bool ok = gfw_dis_check(I, why, sizeof(why));
    if (ok || !strstr(why, text)) { fprintf(stderr, "expected a refusal with \"%s\", got %s \"%s\"\n", text, ok ? "acceptance" : "", why); return false; }
    return true;
}

// the published rule as it is written, in floating point
static int coarsest_rule(int w, int h) {
    const double big = w > h ? w : h, small = w > h ? h : w;
    const int a = (int)(log2(big / 32.0) + 0.5), b = (int)log2(small / 8.0);
    return a < b ? a : b;
}

static void test_levels() {
    int lw[GFW_DIS_LEVELS], lh[GFW_DIS_LEVELS];
    CHECK(gfw_dis_levels(200, 168, lw, lh) == 3 && lw[1] == 100 && lh[1] == 84 && lw[2] == 50 && lh[2] == 42 && lw[3] == 25 && lh[3] == 21 && lw[4] == 0);
    CHECK(gfw_dis_levels(384, 216, lw, lh) == 4 && lw[3] == 48 && lh[3] == 27 && lw[4] == 24 && lh[4] == 13);
    CHECK(gfw_dis_levels(96, 64, lw, lh) == 2 && lw[2] == 24 && lh[2] == 16);
    CHECK(gfw_dis_levels(256, 24, lw, lh) == 1 && lw[1] == 128 && lh[1] == 12);
    CHECK(gfw_dis_coarsest(1280, 720) == 5 && gfw_dis_coarsest(8192, 8192) == 8 && gfw_dis_coarsest(8192, 16) == 1 && gfw_dis_coarsest(7, 7) < 0);
    // the integer form equals the rule wherever a finest scale can be served (>= 1), and is under 1 wherever the rule is
    for (int w = 1; w <= 8192; w += (w < 600 ? 1 : 97))
        for (int h = 1; h <= 8192; h += (h < 600 ? 7 : 331)) {
            const int want = coarsest_rule(w, h), got = gfw_dis_coarsest(w, h);
            if (want >= 1 || got >= 1) CHECK(want == got);
        }
    // the coarsest level always holds a patch
    for (int w = 16; w <= 8192; w += 61) { const int c = gfw_dis_levels(w, 8192 - w / 2, lw, lh); CHECK(c < GFW_DIS_LEVELS && (c < 0 || (lw[c] >= 8 && lh[c] >= 8))); }
    CHECK(gfw_dis_patches(25, 21) == 5 * 4 && gfw_dis_patches(24, 13) == 5 * 2 && gfw_dis_patches(8, 8) == 1 && gfw_dis_patches(320, 180) == 79 * 44);
}

static void test_check() {
    Call c = make_call(3, {0, 1, 1, 2, 0, 2});
    char why[256] = "";
    CHECK(gfw_dis_check(c.inputs(), why, sizeof(why)));
    { Call x = c; x.finest = 1; CHECK(gfw_dis_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.reserved = 1; CHECK(refused(x.inputs(), "reserved")); }
    { Call x = c; x.variational = 5; CHECK(refused(x.inputs(), "variational_iters 5")); }
    { Call x = c; x.finest = 3; CHECK(refused(x.inputs(), "finest_scale 3")); }
    { Call x = c; x.finest = 0; CHECK(refused(x.inputs(), "finest_scale 0")); }
    { Call x = c; x.w = 256; x.h = 24; x.stride = 256; CHECK(refused(x.inputs(), "frames of 256 x 24 have the coarsest scale 1, under the finest scale 2")); }
    { Call x = c; x.w = 256; x.h = 24; x.stride = 256; x.finest = 1; x.on_device = 1; CHECK(gfw_dis_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.w = 0; CHECK(refused(x.inputs(), "frames of 0 x 168")); }
    { Call x = c; x.h = 8193; CHECK(refused(x.inputs(), "frames of 200 x 8193")); }
    { Call x = c; x.stride = 199; CHECK(refused(x.inputs(), "stride 199 under the width 200")); }
    { GfwDisInputs I = c.inputs(); I.n_pairs = -1; CHECK(refused(I, "negative count")); }
    { GfwDisInputs I = c.inputs(); I.n_frames = -1; CHECK(refused(I, "negative count")); }
    { GfwDisInputs I = c.inputs(); I.n_frames = GFW_DIS_FRAMES_MAX + 1; CHECK(refused(I, "4097 frames")); }
    { GfwDisInputs I = c.inputs(); I.n_pairs = GFW_DIS_PAIRS_MAX + 1; CHECK(refused(I, "65536 pairs")); }
    { GfwDisInputs I = c.inputs(); I.pair_frames = nullptr; CHECK(refused(I, "without pair_frames")); }
    { GfwDisInputs I = c.inputs(); I.frames = nullptr; CHECK(refused(I, "without their planes")); }
    { Call x = c; x.pairs[3] = 3; CHECK(refused(x.inputs(), "pair 1: frames (1, 3) outside the call's 3 frames")); }
    { Call x = c; x.pairs[4] = -1; CHECK(refused(x.inputs(), "pair 2: frames (-1, 2) outside")); }
    { Call x = c; x.pairs[5] = 0; CHECK(refused(x.inputs(), "pair 2: frame 0 paired with itself")); }
    { Call x = c; x.w = 16; x.stride = 16; x.h = 8192; x.finest = 1; CHECK(refused(x.inputs(), "has 131072 nodes")); }
    // the 2 GiB of one staged block: host frames of a huge stride are refused without being read (the vector holds three small frames); device frames are not staged
    { Call x = c; x.stride = 1 << 20; x.h = 3000; CHECK(refused(x.inputs(), "at most 2 GiB")); }
    { Call x = c; x.stride = 1 << 20; x.h = 3000; x.on_device = 1; CHECK(gfw_dis_check(x.inputs(), why, sizeof(why))); }
    // the 16 GiB of work space: 8192 x 4096 at the finest scale 1 has a dense field of 64 MiB a pair and 1024 nodes a frame
    { Call x = c; x.w = 8192; x.h = 4096; x.stride = 8192; x.finest = 1; x.on_device = 1; x.pairs.clear(); for (int p = 0; p < 300; ++p) { x.pairs.push_back(p % 3); x.pairs.push_back((p + 1) % 3); }
      CHECK(refused(x.inputs(), "of device work space")); }
    // no pairs: accepted whatever else is null
    { GfwDisInputs I = c.inputs(); I.n_pairs = 0; I.pair_frames = nullptr; I.frames = nullptr; CHECK(gfw_dis_check(I, why, sizeof(why))); }
}

static void stage(const Call &c) {
    const GfwDisInputs I = c.inputs();
    char why[256] = "";
    CHECK(gfw_dis_check(I, why, sizeof(why)));
    const GfwDisPlan P = gfw_dis_plan(I);
    char *block = (char *)malloc(P.total ? P.total : 1);
    memset(block, 0xEE, P.total);
    GfwDisArgs A;
    GfwFlowArgs G;
    memset(&A, 0, sizeof(A));
    memset(&G, 0, sizeof(G));
    gfw_dis_fill(P, I, block, D, WORK, A, G);
    const int n_pairs = I.n_pairs, n_frames = I.n_frames;
    CHECK(memcmp(block + P.o_pairs, c.pairs.data(), sizeof(int32_t) * c.pairs.size()) == 0 && (const char *)A.pair_frames == D + P.o_pairs);
    CHECK(A.n_pairs == n_pairs && A.n_frames == n_frames && A.finest == c.finest && A.coarsest == P.coarsest && A.grid_nodes == P.grid.nodes);
    CHECK(P.points_max == (int64_t)P.grid.nodes * n_pairs);
    if (c.on_device) CHECK(A.lv[0].base == c.frames.data() && P.o_frames + 0 == P.total);
    else { CHECK((const char *)A.lv[0].base == D + P.o_frames && memcmp(block + P.o_frames, c.frames.data(), c.frames.size()) == 0 && P.total >= P.o_frames + c.frames.size()); }
    CHECK(A.lv[0].w == c.w && A.lv[0].h == c.h && A.lv[0].stride == c.stride && A.lv[0].frame_bytes == (int64_t)c.stride * c.h);
    // what the grid launch takes: level 0 and the grid of gfw_flow_pyrlk's point mode 1
    const GfwFlowGrid g = gfw_flow_grid(c.w, c.h);
    CHECK(G.lv[0].base == A.lv[0].base && G.lv[0].w == c.w && G.lv[0].h == c.h && G.lv[0].stride == c.stride && G.lv[0].frame_bytes == A.lv[0].frame_bytes);
    CHECK(G.mode == GFW_FLOW_MODE_GRID && G.n_frames == n_frames && G.grid_step == g.step && G.grid_half == g.half && G.grid_rows == g.rows && G.grid_nodes == g.nodes);
    // the work space: every array inside it, none overlapping the one before
    size_t at = 0;
    for (int l = 1; l < GFW_DIS_LEVELS; ++l) {
        if (l > P.coarsest) { CHECK(!A.lv[l].base && A.lv[l].w == 0 && !A.dense[l]); continue; }
        CHECK((const char *)A.lv[l].base == WORK + P.level_at[l] && P.level_at[l] >= at && P.level_at[l] % 8 == 0);
        CHECK(A.lv[l].w == P.lw[l] && A.lv[l].h == P.lh[l] && A.lv[l].stride == P.lw[l] && A.lv[l].frame_bytes == (int64_t)P.lw[l] * P.lh[l]);
        CHECK(P.lw[l] == P.lw[l - 1] / 2 && P.lh[l] == P.lh[l - 1] / 2 && P.lw[l] >= 8 && P.lh[l] >= 8);
        at = P.level_at[l] + (size_t)n_frames * P.lw[l] * P.lh[l];
    }
    for (int l = 0; l < GFW_DIS_LEVELS; ++l) {
        if (l < c.finest || l > P.coarsest) { CHECK(!A.dense[l] && P.dense_bytes[l] == 0); continue; }
        CHECK((char *)A.dense[l] == WORK + P.dense_at[l] && P.dense_at[l] >= at && P.dense_at[l] % 8 == 0);
        CHECK(P.dense_bytes[l] == sizeof(float) * 2 * (size_t)n_pairs * P.lw[l] * P.lh[l]);
        at = P.dense_at[l] + P.dense_bytes[l];
    }
    size_t most = 0;
    for (int l = c.finest; l <= P.coarsest; ++l) { const size_t n = (size_t)gfw_dis_patches(P.lw[l], P.lh[l]); if (n > most) most = n; }
    CHECK(most == (size_t)gfw_dis_patches(P.lw[c.finest], P.lh[c.finest]));               // the finest level has the most patches
    for (int k = 0; k < 3; ++k) {
        CHECK((char *)A.patch[k] == WORK + P.patch_at[k] && P.patch_at[k] >= at && P.patch_at[k] % 8 == 0);
        at = P.patch_at[k] + sizeof(float) * 2 * (size_t)n_pairs * most;
    }
    CHECK(P.work_bytes >= at);
    free(block);
}

static void test_staging() {
    Call c = make_call(3, {0, 1, 1, 2, 0, 2, 2, 0});
    stage(c);
    { Call x = c; x.on_device = 1; stage(x); }
    { Call x = c; x.finest = 1; stage(x); }
    { Call x = make_call(2, {1, 0}); x.w = 96; x.h = 64; x.stride = 100; x.frames.resize(2 * 100 * 64); stage(x); }      // a single level
    { Call x = make_call(2, {0, 1}); x.w = 384; x.h = 216; x.stride = 384; x.frames.resize(2 * 384 * 216); stage(x); }
}

int main() {
    test_levels();
    test_check();
    test_staging();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("dis host code ok\n");
    return 0;
}
