// test_pose_essential_host.cpp — TEST INFRASTRUCTURE: gfw_pose_essential's host code (gfw_pose_essential_host.h: the check, the staging, the call's constants) and
// gfw_pose_draws_k's generator (gfw_pose_host.h) in a program of their own, built with AddressSanitizer and UBSan (tests/test_cpp_pose_essential_host.py; host pass
// only, no device, no library).  The packer fills a heap block of EXACTLY its layout's total — one byte more is the sanitizer's — at a fake device base; the
// caller's arrays are heap blocks of exactly their sizes too, so a check or a draw that reads or writes past them shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_pose.h"
#include "../../gyroflow_amd/csrc/gfw_pose_host.h"
#include "../../gyroflow_amd/csrc/gfw_pose_essential.h"
#include "../../gyroflow_amd/csrc/gfw_pose_essential_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static const char *const D = (const char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced

struct Call {
    std::vector<int32_t> first, octets;
    std::vector<float> a, b;
    int iters;
    GfwPoseEssInputs inputs() const { return GfwPoseEssInputs{first.data(), a.data(), b.data(), (int)first.size() - 1, octets.data(), iters}; }
};
static Call make_call(const std::vector<int> &counts, int iters, uint64_t seed) {
    Call c;
    c.iters = iters;
    c.first.push_back(0);
    for (int n : counts) c.first.push_back(c.first.back() + n);
    c.a.resize((size_t)c.first.back() * 2); c.b.resize(c.a.size());
    for (size_t i = 0; i < c.a.size(); ++i) { c.a[i] = (float)i; c.b[i] = (float)i + 0.5f; }
    c.octets.assign(counts.size() * (size_t)iters * 8, -9);
    CHECK(gfw_pose_draws_k_host(seed, c.first.data(), (int)counts.size(), iters, 8, c.octets.data()));
    return c;
}

static void test_draws() {
    const std::vector<int> counts = {0, 1, 7, 8, 9, 12, 65, 200, 4096};
    std::vector<int32_t> first{0};
    for (int n : counts) first.push_back(first.back() + n);
    for (int k : {1, 3, 8, 16}) {
        std::vector<int32_t> t(counts.size() * 7 * (size_t)k, -9);
        CHECK(gfw_pose_draws_k_host(11, first.data(), (int)counts.size(), 7, k, t.data()));
        for (size_t p = 0; p < counts.size(); ++p) {
            const int n = counts[p];
            for (int it = 0; it < 7; ++it) {
                const int32_t *o = t.data() + (p * 7 + (size_t)it) * (size_t)k;
                for (int j = 0; j < k; ++j) {
                    if (n < k) { CHECK(o[j] == 0); continue; }                     // a pair under k points: zeros
                    CHECK(o[j] >= 0 && o[j] < n);                                  // in range ..
                    for (int i = 0; i < j; ++i) CHECK(o[i] != o[j]);               // .. and distinct within the tuple
                }
            }
        }
    }
    // k = 8 from n = 8: every round a permutation of 0 .. 7, and rounds differ
    { const int32_t f[2] = {0, 8}; std::vector<int32_t> t(5 * 8, -9); CHECK(gfw_pose_draws_k_host(3, f, 1, 5, 8, t.data()));
      for (int it = 0; it < 5; ++it) { int seen = 0; for (int j = 0; j < 8; ++j) seen |= 1 << t[(size_t)it * 8 + j]; CHECK(seen == 255); }
      CHECK(memcmp(t.data(), t.data() + 8, 32) != 0); }
    // k = 3: gfw_pose_draws' triples to the bit
    { std::vector<int32_t> t3(counts.size() * 7 * 3, -9), tr(counts.size() * 7 * 3, -8);
      CHECK(gfw_pose_draws_k_host(11, first.data(), (int)counts.size(), 7, 3, t3.data()));
      CHECK(gfw_pose_draws_host(11, first.data(), (int)counts.size(), 7, 1000, tr.data(), nullptr, nullptr));
      CHECK(t3 == tr); }
    const Call a = make_call({12, 65}, 5, 1), b = make_call({12, 65}, 5, 1), d = make_call({12, 65}, 5, 2);
    CHECK(a.octets == b.octets);                                                   // a function of the seed ..
    CHECK(a.octets != d.octets);                                                   // .. and not of nothing
    char why[256];
    CHECK(gfw_pose_ess_check(a.inputs(), why, sizeof(why)));                       // what the generator draws, the entry point accepts
    std::vector<int32_t> out((size_t)2 * 5 * 16, -9);
    const int32_t down[3] = {0, 5, 2}, big[2] = {0, 4097};
    CHECK(!gfw_pose_draws_k_host(1, down, 2, 5, 8, out.data()));
    CHECK(!gfw_pose_draws_k_host(1, big, 1, 5, 8, out.data()));
    CHECK(!gfw_pose_draws_k_host(1, a.first.data(), 2, -1, 8, out.data()));
    CHECK(!gfw_pose_draws_k_host(1, a.first.data(), 2, 5, 0, out.data()));
    CHECK(!gfw_pose_draws_k_host(1, a.first.data(), 2, 5, GFW_POSE_DRAWS_K_MAX + 1, out.data()));
    CHECK(!gfw_pose_draws_k_host(1, a.first.data(), 2, 5, 8, nullptr));
    CHECK(gfw_pose_draws_k_host(1, nullptr, 0, 5, 8, nullptr));
}

static void test_check() {
    char why[256];
    Call c = make_call({12, 65, 7}, 4, 3);
    CHECK(gfw_pose_ess_check(c.inputs(), why, sizeof(why)));
    why[0] = 0;
    { Call x = c; x.octets[(1 * 4 + 2) * 8 + 5] = 65; CHECK(!gfw_pose_ess_check(x.inputs(), why, sizeof(why)) && strstr(why, "pair 1: round 2 draws 65 outside its 65 points")); }
    { Call x = c; x.octets[(1 * 4 + 3) * 8 + 7] = -1; CHECK(!gfw_pose_ess_check(x.inputs(), why, sizeof(why)) && strstr(why, "pair 1: round 3 draws -1")); }
    { Call x = c; x.octets[7] = x.octets[0]; CHECK(!gfw_pose_ess_check(x.inputs(), why, sizeof(why)) && strstr(why, "pair 0: round 0 draws a point twice")); }
    { Call x = c; x.octets[(2 * 4) * 8] = 77; CHECK(gfw_pose_ess_check(x.inputs(), why, sizeof(why))); }       // a pair under 8 points: its octets are not read
    { Call x = c; x.first[2] = 5; CHECK(!gfw_pose_ess_check(x.inputs(), why, sizeof(why)) && strstr(why, "pair 1: pair_first descends")); }
    { Call x = c; x.first[0] = -1; CHECK(!gfw_pose_ess_check(x.inputs(), why, sizeof(why)) && strstr(why, "pair 0: pair_first -1 is negative")); }
    { Call x = c; x.first[1] = 4097; x.first[2] = 4100; x.first[3] = 4100; CHECK(!gfw_pose_ess_check(x.inputs(), why, sizeof(why)) && strstr(why, "pair 0: 4097 points")); }
    { GfwPoseEssInputs i = c.inputs(); i.n_pairs = -1; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "negative count")); }
    { GfwPoseEssInputs i = c.inputs(); i.num_iters = -1; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "negative count")); }
    { GfwPoseEssInputs i = c.inputs(); i.num_iters = GFW_PE_ROUNDS_MAX + 1; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "at most 1024")); }
    { GfwPoseEssInputs i = c.inputs(); i.n_pairs = GFW_PE_PAIRS_MAX + 1; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "at most 65535")); }
    { GfwPoseEssInputs i = c.inputs(); i.octets = nullptr; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "rounds without octets")); }
    { GfwPoseEssInputs i = c.inputs(); i.points_b = nullptr; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "without points_a / points_b")); }
    { GfwPoseEssInputs i = c.inputs(); i.pair_first = nullptr; CHECK(!gfw_pose_ess_check(i, why, sizeof(why)) && strstr(why, "without pair_first")); }
    { GfwPoseEssInputs i = c.inputs(); i.n_pairs = 0; i.pair_first = nullptr; i.octets = nullptr; CHECK(gfw_pose_ess_check(i, why, sizeof(why))); }
    char tiny[8];
    { Call x = c; x.first[2] = 5; CHECK(!gfw_pose_ess_check(x.inputs(), tiny, sizeof(tiny)) && strlen(tiny) == 7); }      // the reason is cut to the caller's room
}

static void test_staging() {
    const Call c = make_call({8, 0, 65, 1}, 6, 5);
    const GfwPoseEssInputs I = c.inputs();
    const GfwPoseEssLayout S = gfw_pose_ess_layout(I);
    CHECK(S.o_first % 8 == 0 && S.o_pts % 8 == 0 && S.o_octets % 8 == 0 && S.total % 8 == 0);
    char *h = (char *)malloc(S.total);
    memset(h, 0xA5, S.total);
    GfwPoseEssArgs A;
    memset(&A, 0, sizeof(A));
    gfw_pose_ess_fill(S, I, h, D, A);
    CHECK((const char *)A.pair_first == D + S.o_first && (const char *)A.points == D + S.o_pts && (const char *)A.octets == D + S.o_octets);
    CHECK(A.n_pairs == 4 && A.total == 74 && A.num_iters == 6);
    CHECK(!memcmp(h + S.o_first, c.first.data(), 5 * 4) && !memcmp(h + S.o_pts, c.a.data(), 74 * 8) && !memcmp(h + S.o_pts + 74 * 8, c.b.data(), 74 * 8));
    CHECK(!memcmp(h + S.o_octets, c.octets.data(), c.octets.size() * 4));
    free(h);
    GfwPoseEssInputs none = {nullptr, nullptr, nullptr, 0, nullptr, 5};
    const GfwPoseEssLayout S0 = gfw_pose_ess_layout(none);
    h = (char *)malloc(S0.total);
    memset(&A, 0, sizeof(A));
    gfw_pose_ess_fill(S0, none, h, D, A);
    CHECK(A.n_pairs == 0 && A.total == 0 && *(int32_t *)(h + S0.o_first) == 0);
    free(h);
    gfw_pose_ess_constants(320, 180, 160, 90, 1e-6, 10, A);
    CHECK(A.vw == 320.0f && A.vh == 180.0f && A.fw == 160.0f && A.fh == 90.0f && A.threshold == 1e-6 && A.min_front == 10);
    CHECK(sizeof(gfw_pose_essential_cfg) == 4 * 6 + 8 + 4 * 2 + 8 * 9);           // no padding: the Python binding's layout
}

// the algebra the kernels and the host share, on the host: a planted essential matrix decomposes into its rotation
static void test_algebra() {
    const double c = 0.9993908270190958, s = 0.03489949670250097;                   // 2 degrees about z
    const double R[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, t[3] = {0.6, 0.0, 0.8};
    const double Tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    double E[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) E[i * 3 + j] = Tx[i * 3] * R[j] + Tx[i * 3 + 1] * R[3 + j] + Tx[i * 3 + 2] * R[6 + j];
    double Ra[9], Rb[9], tv[3];
    gfw_pe_rotations(E, Ra, Rb, tv);
    double da = 0.0, db = 0.0;
    for (int i = 0; i < 9; ++i) { da += (Ra[i] - R[i]) * (Ra[i] - R[i]); db += (Rb[i] - R[i]) * (Rb[i] - R[i]); }
    CHECK(da < 1e-24 || db < 1e-24);
    CHECK(fabs(fabs(tv[0] * t[0] + tv[1] * t[1] + tv[2] * t[2]) - 1.0) < 1e-12);
    float q[4];
    gfw_pe_quat(R, q);
    CHECK(fabsf(q[0] - 0.99984770f) < 1e-6f && q[1] == 0.0f && q[2] == 0.0f && fabsf(q[3] - 0.01745241f) < 1e-6f);
    const double half[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1};                           // half a turn about z: the last branch
    gfw_pe_quat(half, q);
    CHECK(q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 1.0f);
}

int main() {
    test_draws();
    test_check();
    test_staging();
    test_algebra();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("pose essential host code ok\n");
    return 0;
}
