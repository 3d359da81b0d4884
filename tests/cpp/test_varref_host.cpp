// test_varref_host.cpp — TEST INFRASTRUCTURE: gfw_flow_dis_refined's host code (gfw_varref_host.h on top of gfw_dis_host.h: the check of the refinement's
// configuration, the work-space plan, a level's argument block, the launch count) in a program of its own, built with AddressSanitizer and UBSan
// (tests/test_cpp_varref_host.py; host pass only, no device, no library).  The work space is a fake device base that is never dereferenced.
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
#include "../../gyroflow_amd/csrc/gfw_varref.h"
#include "../../gyroflow_amd/csrc/gfw_varref_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static char *const D = (char *)(uintptr_t)0x500000000000ull;     // the "device" side of the staged block: never dereferenced
static char *const WORK = (char *)(uintptr_t)0x600000000000ull;  // the DIS plan's work space
static char *const VWORK = (char *)(uintptr_t)0x700000000000ull; // the refinement's

struct Call {
    int w = 200, h = 168, stride = 208, finest = 2, variational = 0, reserved = 0, n_frames = 3;
    std::vector<uint8_t> frames;
    std::vector<int32_t> pairs = {0, 1, 1, 2, 0, 2};
    GfwVarrefInputs V = {5, 5, 20.0f, 5.0f, 10.0f, 1.6f, {0, 0}};
    Call() : frames((size_t)3 * 208 * 168, 9) {}
    GfwDisInputs inputs() const { return GfwDisInputs{w, h, stride, finest, variational, reserved, frames.data(), 1, n_frames, pairs.data(), (int)pairs.size() / 2}; }
};
static bool refused(const Call &c, const char *text) {
    char why[384] = "";
    const bool ok = gfw_varref_check(c.inputs(), c.V, why, sizeof(why));
    if (ok || !strstr(why, text)) { fprintf(stderr, "expected a refusal with \"%s\", got %s \"%s\"\n", text, ok ? "acceptance" : "", why); return false; }
    return true;
}

static void test_check() {
    Call c;
    char why[384] = "";
    CHECK(gfw_varref_check(c.inputs(), c.V, why, sizeof(why)));
    { Call x = c; x.V.fixed_point_iters = 0; CHECK(gfw_varref_check(x.inputs(), x.V, why, sizeof(why))); }
    { Call x = c; x.V.fixed_point_iters = 64; x.V.sor_iters = 64; CHECK(gfw_varref_check(x.inputs(), x.V, why, sizeof(why))); }
    { Call x = c; x.V.omega = 1.9999f; CHECK(gfw_varref_check(x.inputs(), x.V, why, sizeof(why))); }
    { Call x = c; x.variational = 5; CHECK(refused(x, "variational_iters 5 in gfw_flow_dis_cfg beside fixed_point_iters 5 in gfw_flow_varref_cfg")); }
    { Call x = c; x.variational = 5; x.V.fixed_point_iters = 0; CHECK(refused(x, "variational_iters 5 in gfw_flow_dis_cfg beside fixed_point_iters 0")); }
    { Call x = c; x.V.fixed_point_iters = -1; CHECK(refused(x, "fixed_point_iters -1 (0 to 64)")); }
    { Call x = c; x.V.fixed_point_iters = 65; CHECK(refused(x, "fixed_point_iters 65 (0 to 64)")); }
    { Call x = c; x.V.sor_iters = 0; CHECK(refused(x, "sor_iters 0 (1 to 64)")); }
    { Call x = c; x.V.sor_iters = 65; CHECK(refused(x, "sor_iters 65 (1 to 64)")); }
    const float bad[] = {0.0f, -1.0f, INFINITY, -INFINITY, NAN};
    for (float b : bad) {
        { Call x = c; x.V.alpha = b; CHECK(refused(x, "alpha")); }
        { Call x = c; x.V.delta = b; CHECK(refused(x, "delta")); }
        { Call x = c; x.V.gamma = b; CHECK(refused(x, "gamma")); }
        { Call x = c; x.V.omega = b; CHECK(refused(x, "omega")); }
    }
    { Call x = c; x.V.omega = 2.0f; CHECK(refused(x, "omega 2 (between 0 and 2, both excluded)")); }
    { Call x = c; x.V.reserved[0] = 1; CHECK(refused(x, "refinement configuration: the reserved slots")); }
    { Call x = c; x.V.reserved[1] = -1; CHECK(refused(x, "refinement configuration: the reserved slots")); }
    // what gfw_dis_check refuses is refused in its words
    { Call x = c; x.reserved = 1; CHECK(refused(x, "bad DIS flow configuration: the reserved slot")); }
    { Call x = c; x.finest = 3; CHECK(refused(x, "finest_scale 3")); }
    { Call x = c; x.pairs[3] = 3; CHECK(refused(x, "pair 1: frames (1, 3) outside the call's 3 frames")); }
    { Call x = c; x.stride = 199; CHECK(refused(x, "stride 199 under the width 200")); }
    // gfw_dis_check's own rejection still carries its words and names the refined call
    { Call x = c; x.variational = 5; CHECK(!gfw_dis_check(x.inputs(), why, sizeof(why)) && strstr(why, "variational_iters 5") && strstr(why, "gfw_flow_dis_refined")); }
    // the 16 GiB hold both work spaces together: 4096 x 4096 at the finest scale 1, 2048 x 2048 pixels a pair at the finest level.  96 pairs: the DIS plan needs
    // about 4.2 GiB and is accepted by gfw_dis_check; the refinement's 17 planes of 1.5 GiB each take the sum over the limit
    { Call x = c; x.w = 4096; x.h = 4096; x.stride = 4096; x.finest = 1; x.pairs.clear(); for (int p = 0; p < 96; ++p) { x.pairs.push_back(p % 3); x.pairs.push_back((p + 1) % 3); }
      CHECK(gfw_dis_check(x.inputs(), why, sizeof(why)));
      CHECK(refused(x, "of device work space"));
      CHECK(!gfw_varref_check(x.inputs(), x.V, why, sizeof(why)) && strstr(why, "(96 pairs, 3 frames of 4096 x 4096 at the finest scale 1") && strstr(why, "at most 16 GiB"));
      Call y = x; y.V.fixed_point_iters = 0; CHECK(gfw_varref_check(y.inputs(), y.V, why, sizeof(why))); }       // no refinement, no work space of its own
    // no pairs: accepted whatever else is null, but not with a bad refinement configuration
    { GfwDisInputs I = c.inputs(); I.n_pairs = 0; I.pair_frames = nullptr; I.frames = nullptr; CHECK(gfw_varref_check(I, c.V, why, sizeof(why)));
      GfwVarrefInputs V = c.V; V.sor_iters = 0; CHECK(!gfw_varref_check(I, V, why, sizeof(why))); }
}

static void test_plan_and_levels() {
    CHECK(gfw_varref_launches(5, 5) == 57 && gfw_varref_launches(2, 3) == 16 && gfw_varref_launches(1, 1) == 5 && gfw_varref_launches(0, 5) == 0 && gfw_varref_launches(64, 64) == 2 + 64 * 129);
    Call c;
    for (int finest = 1; finest <= 2; ++finest) {
        c.finest = finest;
        const GfwDisInputs I = c.inputs();
        const GfwDisPlan P = gfw_dis_plan(I);
        const GfwVarrefPlan VP = gfw_varref_plan(I, P, c.V);
        CHECK(VP.levels == P.coarsest - finest + 1 && VP.launches == 57 * VP.levels);
        CHECK(VP.plane_bytes == sizeof(float) * 3 * (size_t)P.lw[finest] * P.lh[finest]);
        size_t at = 0;
        for (int k = 0; k < GFW_VARREF_PLANES; ++k) { CHECK(VP.plane_at[k] >= at && VP.plane_at[k] % 8 == 0); at = VP.plane_at[k] + VP.plane_bytes; }
        CHECK(VP.work_bytes >= at && GFW_VARREF_PLANES == 17);
        GfwDisArgs A;
        GfwFlowArgs G;
        memset(&A, 0, sizeof(A)); memset(&G, 0, sizeof(G));
        std::vector<char> block(P.total ? P.total : 1);
        gfw_dis_fill(P, I, block.data(), D, WORK, A, G);
        for (int l = finest; l <= P.coarsest; ++l) {
            const GfwVarrefArgs R = gfw_varref_level(VP, c.V, A, l, VWORK);
            CHECK(R.base == A.lv[l].base && R.frame_bytes == A.lv[l].frame_bytes && R.w == P.lw[l] && R.h == P.lh[l] && R.stride == A.lv[l].stride && R.n_pairs == 3);
            CHECK(R.pair_frames == A.pair_frames && R.U == A.dense[l] && R.w >= 8 && R.h >= 8);
            CHECK(R.alpha == 20.0f && R.delta == 5.0f && R.gamma == 10.0f && R.omega == 1.6f);
            // every plane holds the level: the finest is the largest
            for (int k = 0; k < GFW_VARREF_PLANES; ++k) CHECK((char *)R.plane[k] == VWORK + VP.plane_at[k] && sizeof(float) * 3 * (size_t)R.w * R.h <= VP.plane_bytes);
        }
    }
    // no fixed-point iteration, or no pairs: no work space and no launch
    { Call x; x.V.fixed_point_iters = 0; const GfwVarrefPlan VP = gfw_varref_plan(x.inputs(), gfw_dis_plan(x.inputs()), x.V); CHECK(VP.work_bytes == 0 && VP.launches == 0 && VP.levels == 0); }
    { Call x; x.pairs.clear(); const GfwVarrefPlan VP = gfw_varref_plan(x.inputs(), gfw_dis_plan(x.inputs()), x.V); CHECK(VP.work_bytes == 0 && VP.launches == 0); }
    // 1280 x 720 at the reference's finest scale: 24 launches become 252
    { Call x; x.w = 1280; x.h = 720; x.stride = 1280; x.frames.assign((size_t)3 * 1280 * 720, 1);
      const GfwDisInputs I = x.inputs(); const GfwDisPlan P = gfw_dis_plan(I); const GfwVarrefPlan VP = gfw_varref_plan(I, P, x.V);
      CHECK(3 + P.coarsest + 4 * (P.coarsest - 2 + 1) == 24 && 24 + VP.launches == 252 && VP.plane_bytes == sizeof(float) * 3 * 320 * 180); }
}

int main() {
    test_check();
    test_plan_and_levels();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("varref host code ok\n");
    return 0;
}
