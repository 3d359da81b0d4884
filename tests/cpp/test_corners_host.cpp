// test_corners_host.cpp — TEST INFRASTRUCTURE: gfw_corners_shi_tomasi's host code (gfw_corners_host.h: the check, the plan with its batches, the staging) in a
// program of its own, built with AddressSanitizer and UBSan (tests/test_cpp_corners_host.py; host pass only, no device, no library).  The packer fills a heap block
// of EXACTLY its plan's total — one byte more is the sanitizer's — at a fake device base; the caller's frames are a heap block of exactly their size too, so a check
// or a fill that reads or writes past them shows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_corners.h"
#include "../../gyroflow_amd/csrc/gfw_corners_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static char *const D = (char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced
static unsigned long long *const CAND = (unsigned long long *)(uintptr_t)0x600000000000ull;
static char OUT[4];                                              // the outputs are only asked whether they are there

struct Call {
    int w = 200, h = 168, stride = 208, max_corners = 200; float quality = 0.01f, min_distance = 10.0f; int mb = 0, reserved = 0, on_device = 0, n = 3;
    std::vector<uint8_t> frames;
    bool packed = true;
    GfwCornersInputs inputs() const {
        return GfwCornersInputs{w, h, stride, max_corners, quality, min_distance, mb, reserved, frames.data(), on_device, n, OUT, OUT, packed ? OUT : nullptr, packed ? OUT : nullptr};
    }
};
static Call make_call(int n, int w = 200, int h = 168, int stride = 208) {
    Call c;
    c.n = n; c.w = w; c.h = h; c.stride = stride;
    c.frames.resize((size_t)n * stride * h);
    for (size_t i = 0; i < c.frames.size(); ++i) c.frames[i] = (uint8_t)(i * 7);
    return c;
}
static bool refused(const GfwCornersInputs &I, const char *text) {
    char why[256] = "";
    const bool ok = gfw_corners_check(I, why, sizeof(why));
    if (ok || !strstr(why, text)) { fprintf(stderr, "expected a refusal with \"%s\", got %s \"%s\"\n", text, ok ? "acceptance" : "", why); return false; }
    return true;
}

static void test_check() {
    const Call c = make_call(3);
    char why[256] = "";
    CHECK(gfw_corners_check(c.inputs(), why, sizeof(why)));
    { Call x = c; x.reserved = 1; CHECK(refused(x.inputs(), "reserved")); }
    { Call x = c; x.w = 2; CHECK(refused(x.inputs(), "frames of 2 x 168")); }
    { Call x = c; x.h = 8193; CHECK(refused(x.inputs(), "frames of 200 x 8193")); }
    { Call x = c; x.stride = 199; CHECK(refused(x.inputs(), "stride 199 under the width 200")); }
    { Call x = c; x.max_corners = 0; CHECK(refused(x.inputs(), "max_corners 0")); }
    { Call x = c; x.max_corners = GFW_CORNERS_MAX + 1; CHECK(refused(x.inputs(), "max_corners 4097")); }
    { Call x = c; x.max_corners = GFW_CORNERS_MAX; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.quality = 0.0f; CHECK(refused(x.inputs(), "quality 0")); }
    { Call x = c; x.quality = 1.0f; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.quality = nextafterf(1.0f, 2.0f); CHECK(refused(x.inputs(), "quality 1")); }
    { Call x = c; x.quality = NAN; CHECK(refused(x.inputs(), "quality nan")); }
    { Call x = c; x.quality = INFINITY; CHECK(refused(x.inputs(), "quality inf")); }
    { Call x = c; x.quality = -0.5f; CHECK(refused(x.inputs(), "quality -0.5")); }
    { Call x = c; x.min_distance = -1.0f; CHECK(refused(x.inputs(), "min_distance -1")); }
    { Call x = c; x.min_distance = 0.0f; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.min_distance = 1024.0f; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); }
    { Call x = c; x.min_distance = 1024.5f; CHECK(refused(x.inputs(), "min_distance 1024.5")); }
    { Call x = c; x.min_distance = NAN; CHECK(refused(x.inputs(), "min_distance nan")); }
    { Call x = c; x.min_distance = INFINITY; CHECK(refused(x.inputs(), "min_distance inf")); }
    { Call x = c; x.mb = -1; CHECK(refused(x.inputs(), "max_workspace_mb -1 is negative")); }
    { Call x = c; x.n = -1; CHECK(refused(x.inputs(), "negative count")); }
    { Call x = c; x.n = GFW_CORNERS_FRAMES_MAX + 1; CHECK(refused(x.inputs(), "4097 frames")); }
    { GfwCornersInputs I = c.inputs(); I.frames = nullptr; CHECK(refused(I, "without their planes")); }
    { GfwCornersInputs I = c.inputs(); I.corners = nullptr; CHECK(refused(I, "null corners / counts")); }
    { GfwCornersInputs I = c.inputs(); I.counts = nullptr; CHECK(refused(I, "null corners / counts")); }
    { GfwCornersInputs I = c.inputs(); I.feat_first = nullptr; CHECK(refused(I, "both or neither")); }
    { GfwCornersInputs I = c.inputs(); I.features = nullptr; CHECK(refused(I, "both or neither")); }
    { Call x = c; x.packed = false; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); }
    // no frames: accepted whatever else is null
    { GfwCornersInputs I = c.inputs(); I.n_frames = 0; I.frames = nullptr; I.corners = nullptr; I.counts = nullptr; I.feat_first = nullptr; CHECK(gfw_corners_check(I, why, sizeof(why))); }
    // a work space too small for one frame names the need: 1998 * 166 * 8 bytes
    { Call x = c; x.w = 2000; x.stride = 2000; x.mb = 2; CHECK(refused(x.inputs(), "the candidate list of ONE 2000 x 168 frame needs 2653344 bytes (3 MB)")); }
    { Call x = c; x.w = 2000; x.stride = 2000; x.mb = 3; x.frames.resize((size_t)3 * 2000 * 168); CHECK(gfw_corners_check(x.inputs(), why, sizeof(why)) && gfw_corners_plan(x.inputs()).n_batches == 3); }
    // the default holds the largest frame; the smallest frame has one slot
    { Call x = c; x.w = x.h = x.stride = 8192; x.on_device = 1; x.n = 2; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); const GfwCornersPlan P = gfw_corners_plan(x.inputs()); CHECK(P.batch_frames == 1 && P.n_batches == 2 && P.list_bytes == (size_t)8190 * 8190 * 8 && P.list_bytes <= P.workspace_cap); }
    { Call x = make_call(2, 3, 3, 3); CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); const GfwCornersPlan P = gfw_corners_plan(x.inputs()); CHECK(P.slots == 1 && P.tiles_x == 1 && P.tiles_y == 1 && P.batch_frames == 2); }
    // the 2 GiB of one staged block: host frames of a huge stride are refused without being read; device frames are not staged
    { Call x = c; x.stride = 1 << 20; x.h = 8192; CHECK(refused(x.inputs(), "at most 2 GiB")); }
    { Call x = c; x.stride = 1 << 20; x.h = 8192; x.on_device = 1; CHECK(gfw_corners_check(x.inputs(), why, sizeof(why))); }
}

static void stage(const Call &c, int want_batches, int want_batch_frames) {
    const GfwCornersInputs I = c.inputs();
    char why[256] = "";
    CHECK(gfw_corners_check(I, why, sizeof(why)));
    const GfwCornersPlan P = gfw_corners_plan(I);
    CHECK(P.n_batches == want_batches && P.batch_frames == want_batch_frames);
    CHECK(P.slots == (int64_t)(c.w - 2) * (c.h - 2) && P.list_bytes == (size_t)P.slots * 8 && P.cand_bytes == P.list_bytes * (size_t)P.batch_frames && P.cand_bytes <= P.workspace_cap);
    CHECK(P.tiles_x * GFW_CORNERS_TILE_W >= c.w && (P.tiles_x - 1) * GFW_CORNERS_TILE_W < c.w && P.tiles_y * GFW_CORNERS_TILE_H >= c.h && (P.tiles_y - 1) * GFW_CORNERS_TILE_H < c.h);
    char *block = (char *)malloc(P.total ? P.total : 1);
    memset(block, 0xEE, P.total);
    GfwCornersArgs A;
    memset(&A, 0, sizeof(A));
    gfw_corners_fill(P, I, block, D, CAND, A);
    for (int f = 0; f < c.n; ++f) CHECK(((const uint32_t *)(block + P.o_max))[f] == 0 && ((const uint32_t *)(block + P.o_count))[f] == 0);
    CHECK((char *)A.max_bits == D + P.o_max && (char *)A.cand_count == D + P.o_count && A.cand == CAND && A.slots == P.slots);
    CHECK(P.o_max % 8 == 0 && P.o_count >= P.o_max + 4 * (size_t)c.n && P.o_frames >= P.o_count + 4 * (size_t)c.n);
    if (c.on_device) CHECK(A.frames == c.frames.data() && P.o_frames == P.total);
    else CHECK((const char *)A.frames == D + P.o_frames && memcmp(block + P.o_frames, c.frames.data(), c.frames.size()) == 0 && P.total >= P.o_frames + c.frames.size());
    CHECK(A.w == c.w && A.h == c.h && A.stride == c.stride && A.frame_bytes == (int64_t)c.stride * c.h && A.n_frames == c.n && A.max_corners == c.max_corners);
    CHECK(A.quality == c.quality && A.min_distance == c.min_distance && A.tiles_x == P.tiles_x && A.tiles_y == P.tiles_y);
    int covered = 0;
    for (int b = 0; b < P.n_batches; ++b) {                         // the batches cover the frames once, in order; only the last one is short
        gfw_corners_batch(P, b, A);
        CHECK(A.frame0 == covered && A.batch_frames >= 1 && A.batch_frames <= P.batch_frames && (b == P.n_batches - 1 || A.batch_frames == P.batch_frames));
        covered += A.batch_frames;
    }
    CHECK(covered == c.n);
    free(block);
}

static void test_staging() {
    stage(make_call(3), 1, 3);
    { Call x = make_call(3); x.on_device = 1; stage(x, 1, 3); }
    { Call x = make_call(5, 384, 216, 384); x.mb = 1; stage(x, 5, 1); }            // 653984 bytes a frame: one fits 1 MiB,
    { Call x = make_call(5, 384, 216, 384); x.mb = 2; stage(x, 2, 3); }            // three fit 2 MiB (3 + 2),
    { Call x = make_call(5, 384, 216, 384); x.mb = 4; stage(x, 1, 5); }            // all five fit 4 MiB
    { Call x = make_call(7, 384, 216, 384); x.mb = 2; x.on_device = 1; stage(x, 3, 3); }
    stage(make_call(1, 3, 3, 5), 1, 1);
    stage(make_call(2, 65, 17, 65), 1, 2);                                          // a pixel more than a tile in both directions
}

int main() {
    test_check();
    test_staging();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("corners host code ok\n");
    return 0;
}
