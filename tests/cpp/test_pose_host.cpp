// test_pose_host.cpp — TEST INFRASTRUCTURE: gfw_pose_almeida's host code (gfw_pose_host.h: the check, the staging, the call's constants) and gfw_pose_draws' generator
// in a program of their own, built with AddressSanitizer and UBSan (tests/test_cpp_pose_host.py; host pass only, no device, no library).  The packer fills a heap
// block of EXACTLY its layout's total — one byte more is the sanitizer's — at a fake device base; the caller's arrays are heap blocks of exactly their sizes too, so a
// check or a draw that reads or writes past them shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_pose.h"
#include "../../gyroflow_amd/csrc/gfw_pose_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static const char *const D = (const char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced

struct Call {
    std::vector<int32_t> first, triples, sample_first, samples;
    std::vector<float> a, b;
    int iters, num_samples;
    GfwPoseInputs inputs(bool lists) const {
        return GfwPoseInputs{first.data(), a.data(), b.data(), (int)first.size() - 1, triples.data(), lists ? sample_first.data() : nullptr, lists ? samples.data() : nullptr, iters, num_samples};
    }
};
static Call make_call(const std::vector<int> &counts, int iters, int num_samples, uint64_t seed) {
    Call c;
    c.iters = iters; c.num_samples = num_samples;
    c.first.push_back(0); c.sample_first.push_back(0);
    for (int n : counts) { c.first.push_back(c.first.back() + n); c.sample_first.push_back(c.sample_first.back() + iters * gfw_pose_list_len(n, num_samples)); }
    c.a.resize((size_t)c.first.back() * 2); c.b.resize(c.a.size());
    for (size_t i = 0; i < c.a.size(); ++i) { c.a[i] = (float)i; c.b[i] = (float)i + 0.5f; }
    c.triples.assign(counts.size() * (size_t)iters * 3, -9);
    c.samples.assign((size_t)c.sample_first.back(), -9);
    CHECK(gfw_pose_draws_host(seed, c.first.data(), (int)counts.size(), iters, num_samples, c.triples.data(), c.sample_first.data(), c.samples.data()));
    return c;
}

static void test_draws() {
    const std::vector<int> counts = {0, 1, 2, 3, 4, 12, 65, 200, 4096};
    for (int num_samples : {40, 1000}) {
        const Call c = make_call(counts, 7, num_samples, 11);
        for (size_t p = 0; p < counts.size(); ++p) {
            const int n = counts[p], m = gfw_pose_list_len(n, num_samples);
            for (int it = 0; it < 7; ++it) {
                const int32_t *t = c.triples.data() + (p * 7 + (size_t)it) * 3;
                if (n < 3) { CHECK(t[0] == 0 && t[1] == 0 && t[2] == 0); }
                else { CHECK(t[0] >= 0 && t[0] < n && t[1] >= 0 && t[1] < n && t[2] >= 0 && t[2] < n); CHECK(t[0] != t[1] && t[0] != t[2] && t[1] != t[2]); }
                std::vector<char> seen((size_t)n + 1, 0);
                const int32_t *s = c.samples.data() + c.sample_first[p] + (size_t)it * m;
                for (int k = 0; k < m; ++k) { CHECK(s[k] >= 0 && s[k] < n); if (s[k] >= 0 && s[k] < n) { CHECK(!seen[(size_t)s[k]]); seen[(size_t)s[k]] = 1; } }      // a permutation prefix
            }
        }
        char why[256];
        CHECK(gfw_pose_check(c.inputs(true), why, sizeof(why)));                 // what the generator draws, the entry point accepts
    }
    const Call a = make_call({12, 65}, 5, 1000, 1), b = make_call({12, 65}, 5, 1000, 1), d = make_call({12, 65}, 5, 1000, 2);
    CHECK(a.triples == b.triples && a.samples == b.samples);                     // a function of the seed ..
    CHECK(a.triples != d.triples && a.samples != d.samples);                     // .. and not of nothing
    std::vector<int32_t> only((size_t)2 * 5 * 3, -9);
    CHECK(gfw_pose_draws_host(1, a.first.data(), 2, 5, 1000, only.data(), nullptr, nullptr) && only == a.triples);      // triples alone
    const int32_t down[3] = {0, 5, 2}, big[2] = {0, 4097};
    CHECK(!gfw_pose_draws_host(1, down, 2, 5, 10, only.data(), nullptr, nullptr));
    CHECK(!gfw_pose_draws_host(1, big, 1, 5, 10, only.data(), nullptr, nullptr));
    CHECK(!gfw_pose_draws_host(1, a.first.data(), 2, -1, 10, only.data(), nullptr, nullptr));
    CHECK(gfw_pose_draws_host(1, nullptr, 0, 5, 10, nullptr, nullptr, nullptr));
}

static void test_check() {
    char why[256];
    Call c = make_call({12, 65, 2}, 4, 40, 3);
    CHECK(gfw_pose_check(c.inputs(true), why, sizeof(why)));
    why[0] = 0;
    CHECK(!gfw_pose_check(c.inputs(false), why, sizeof(why)) && strstr(why, "pair 1: 65 points but num_samples 40"));
    { Call x = c; x.triples[(1 * 4 + 2) * 3 + 1] = 65; CHECK(!gfw_pose_check(x.inputs(true), why, sizeof(why)) && strstr(why, "pair 1: round 2")); }
    { Call x = c; x.triples[0] = x.triples[1]; CHECK(!gfw_pose_check(x.inputs(true), why, sizeof(why)) && strstr(why, "pair 0: round 0 draws a point twice")); }
    { Call x = c; x.triples[(2 * 4) * 3] = 77; CHECK(gfw_pose_check(x.inputs(true), why, sizeof(why))); }       // a pair under 3 points: its triples are not read
    { Call x = c; x.samples[(size_t)x.sample_first[2] - 1] = -1; CHECK(!gfw_pose_check(x.inputs(true), why, sizeof(why)) && strstr(why, "pair 1: sample -1 of round 3")); }
    { Call x = c; x.sample_first[1] -= 1; CHECK(!gfw_pose_check(x.inputs(true), why, sizeof(why)) && strstr(why, "pair 0: 47 sample entries")); }
    { Call x = c; x.first[2] = 5; CHECK(!gfw_pose_check(x.inputs(true), why, sizeof(why)) && strstr(why, "pair 1: pair_first descends")); }
    { GfwPoseInputs i = c.inputs(true); i.n_pairs = -1; CHECK(!gfw_pose_check(i, why, sizeof(why)) && strstr(why, "negative count")); }
    { GfwPoseInputs i = c.inputs(true); i.num_iters = GFW_POSE_ROUNDS_MAX + 1; CHECK(!gfw_pose_check(i, why, sizeof(why)) && strstr(why, "at most 1024")); }
    { GfwPoseInputs i = c.inputs(true); i.n_pairs = 0; i.pair_first = nullptr; i.triples = nullptr; CHECK(gfw_pose_check(i, why, sizeof(why))); }
    char tiny[8];
    { Call x = c; x.first[2] = 5; CHECK(!gfw_pose_check(x.inputs(true), tiny, sizeof(tiny)) && strlen(tiny) == 7); }      // the reason is cut to the caller's room
}

static void test_staging() {
    for (int lists = 0; lists < 2; ++lists) {
        const Call c = make_call({3, 0, 65, 1}, 6, lists ? 40 : 1000, 5);
        // the arrays may start inside the caller's: sample_first[0] above 0
        std::vector<int32_t> sf = c.sample_first, sm(7, -5);
        for (int32_t &v : sf) v += 7;
        sm.insert(sm.end(), c.samples.begin(), c.samples.end());
        GfwPoseInputs I = c.inputs(lists != 0);
        if (lists) { I.sample_first = sf.data(); I.samples = sm.data(); }
        const GfwPoseLayout S = gfw_pose_layout(I);
        CHECK(S.o_first % 8 == 0 && S.o_pts % 8 == 0 && S.o_triples % 8 == 0 && S.o_sfirst % 8 == 0 && S.o_samples % 8 == 0 && S.total % 8 == 0);
        char *h = (char *)malloc(S.total);
        memset(h, 0xA5, S.total);
        GfwPoseArgs A;
        memset(&A, 0, sizeof(A));
        gfw_pose_fill(S, I, h, D, A);
        CHECK((const char *)A.pair_first == D + S.o_first && (const char *)A.points == D + S.o_pts && (const char *)A.triples == D + S.o_triples);
        CHECK(A.n_pairs == 4 && A.total == 69 && A.num_iters == 6 && A.num_samples == (lists ? 40 : 1000));
        CHECK(!memcmp(h + S.o_first, c.first.data(), 5 * 4) && !memcmp(h + S.o_pts, c.a.data(), 69 * 8) && !memcmp(h + S.o_pts + 69 * 8, c.b.data(), 69 * 8));
        CHECK(!memcmp(h + S.o_triples, c.triples.data(), c.triples.size() * 4));
        if (lists) {
            CHECK((const char *)A.sample_first == D + S.o_sfirst && (const char *)A.samples == D + S.o_samples);
            CHECK(!memcmp(h + S.o_sfirst, c.sample_first.data(), 5 * 4) && !memcmp(h + S.o_samples, c.samples.data(), c.samples.size() * 4));      // staged from 0
        } else CHECK(!A.sample_first && !A.samples);
        free(h);
    }
    GfwPoseInputs none = {nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 5, 10};
    const GfwPoseLayout S = gfw_pose_layout(none);
    char *h = (char *)malloc(S.total);
    GfwPoseArgs A;
    memset(&A, 0, sizeof(A));
    gfw_pose_fill(S, none, h, D, A);
    CHECK(A.n_pairs == 0 && A.total == 0 && *(int32_t *)(h + S.o_first) == 0);
    free(h);
    const double K[9] = {150.5, 0.0, 160.25, 0.0, 151.5, 90.75, 0.0, 0.0, 1.0};
    gfw_pose_constants(320, 180, 160, 90, 0.05f, K, A);
    CHECK(A.vw == 320.0f && A.vh == 180.0f && A.fw == 160.0f && A.fh == 90.0f && A.fx == 150.5f && A.fy == 151.5f && A.cx == 160.25f && A.cy == 90.75f);
    CHECK(A.target > 8.72e-4f && A.target < 8.73e-4f && A.K[4] == 151.5);
    // the derivative matrices are K times a rotation by a thousandth of a degree: K itself to a few parts in 10^5, and not K
    for (int k = 0; k < 3; ++k) for (int i = 0; i < 9; ++i) CHECK(A.eps_m[k * 9 + i] > (float)K[i] - 0.01f && A.eps_m[k * 9 + i] < (float)K[i] + 0.01f);
    CHECK(A.eps_m[2] != (float)K[2] && A.eps_m[9 + 5] != (float)K[5] && A.eps_m[18 + 1] != 0.0f);
}

int main() {
    test_draws();
    test_check();
    test_staging();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("pose host code ok\n");
    return 0;
}
