// test_rs_sync_host.cpp — TEST INFRASTRUCTURE: gfw_sync_rs_costs' / gfw_sync_rs_search's host code (gfw_sync_rs_host.h: the check that names the range or pair, the
// staging, the call's constants, the round schedule) and the host side of the track lookup (gfw_sync_rs.h) in a program of their own, built with AddressSanitizer
// and UBSan (tests/test_cpp_rs_sync_host.py; host pass only, no device, no library).  The packer fills a heap block of EXACTLY its layout's total — one byte more is
// the sanitizer's — at a fake device base; the caller's arrays and the track are heap blocks of exactly their sizes too, so a check, a fill or a lookup that reads
// or writes past them shows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_sync_rs.h"
#include "../../gyroflow_amd/csrc/gfw_sync_rs_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static const char *const D = (const char *)(uintptr_t)0x500000000000ull;     // the "device" side of the block: never dereferenced

struct Call {
    std::vector<int32_t> range_first, pair_first, cand_first;
    std::vector<int64_t> pair_ts, track_ts;
    std::vector<float> a, b;
    std::vector<double> track_q, cand;
    GfwRsInputs inputs(bool search) const {
        return GfwRsInputs{range_first.data(), (int)range_first.size() - 1, pair_ts.data(), pair_first.data(), a.data(), b.data(), (int)pair_first.size() - 1,
                           track_ts.data(), track_q.data(), (int)track_ts.size(), search ? nullptr : cand_first.data(), search ? nullptr : cand.data(), search ? 0 : (int)cand.size()};
    }
};
// ranges of {3, 0, 2} pairs; pairs of {0, 1, 64, 65, 7} points; the points start at `lead` of the caller's arrays; a track of 9 samples
static Call make_call(int lead) {
    Call c;
    c.range_first = {0, 3, 3, 5};
    c.pair_first.push_back(lead);
    for (int n : {0, 1, 64, 65, 7}) c.pair_first.push_back(c.pair_first.back() + n);
    for (int p = 0; p < 5; ++p) { c.pair_ts.push_back(1000000 + 33333 * p); c.pair_ts.push_back(1000000 + 33333 * (p + 1)); }
    c.a.resize((size_t)c.pair_first.back() * 2); c.b.resize(c.a.size());
    for (size_t i = 0; i < c.a.size(); ++i) { c.a[i] = (float)i; c.b[i] = (float)i + 0.5f; }
    for (int i = 0; i < 9; ++i) { c.track_ts.push_back(500000 + 250000ll * i); c.track_q.insert(c.track_q.end(), {1.0, 0.01 * i, 0.0, 0.0}); }
    c.cand_first = {0, 4, 6, 7};
    for (int i = 0; i < 7; ++i) c.cand.push_back(0.001 * i);
    return c;
}
static GfwRsSettings settings(bool search) {
    GfwRsSettings S;
    memset(&S, 0, sizeof(S));
    S.step_s = 0.003; S.initial_delay_s = 0.0; S.radius_s = 0.03; S.loss_scale = 1000.0; S.rounds = 4; S.refine = 1; S.hypotheses = 16; S.refits = 3; S.sweeps = 8; S.search = search;
    return S;
}
static bool refused(const GfwRsInputs &I, const GfwRsSettings &S, const char *text) {
    char why[256] = "";
    const bool ok = gfw_rs_check(I, S, why, sizeof(why));
    if (ok || !strstr(why, text)) fprintf(stderr, "expected a refusal with '%s', got %s '%s'\n", text, ok ? "acceptance" : "refusal", why);
    return !ok && strstr(why, text);
}

static void test_check() {
    char why[256];
    for (int search = 0; search < 2; ++search) {
        const Call c = make_call(search ? 0 : 6);
        CHECK(gfw_rs_check(c.inputs(search != 0), settings(search != 0), why, sizeof(why)));
        { Call x = c; x.range_first = {1, 3, 3, 5}; CHECK(refused(x.inputs(search != 0), settings(search != 0), "range 0: range_first 1 is not 0")); }
        { Call x = c; x.range_first = {0, 3, 2, 5}; CHECK(refused(x.inputs(search != 0), settings(search != 0), "range 1: range_first descends")); }
        { Call x = c; x.range_first = {0, 3, 3, 4}; CHECK(refused(x.inputs(search != 0), settings(search != 0), "range 2: range_first ends at 4, the call has 5 pairs")); }
        { Call x = c; x.pair_first[3] = x.pair_first[2] - 1; CHECK(refused(x.inputs(search != 0), settings(search != 0), "pair 2: pair_first descends")); }
        { Call x = c; x.pair_first[0] = -1; CHECK(refused(x.inputs(search != 0), settings(search != 0), "pair 0: pair_first -1 is negative")); }
        { Call x = c; for (size_t p = 3; p < x.pair_first.size(); ++p) x.pair_first[p] += 4096; CHECK(refused(x.inputs(search != 0), settings(search != 0), "pair 2: 4160 points, at most 4096")); }
        { Call x = c; x.track_ts[4] = x.track_ts[3]; CHECK(refused(x.inputs(search != 0), settings(search != 0), "track sample 4: timestamp")); }
        { Call x = c; x.track_ts.resize(1); x.track_q.resize(4); CHECK(refused(x.inputs(search != 0), settings(search != 0), "a track of 1 samples: at least 2")); }
        { GfwRsInputs I = c.inputs(search != 0); I.points_b = nullptr; CHECK(refused(I, settings(search != 0), "without points_a / points_b")); }
        { GfwRsInputs I = c.inputs(search != 0); I.n_pairs = GFW_RS_PAIRS_MAX + 1; CHECK(refused(I, settings(search != 0), "at most 65535")); }
        { GfwRsSettings S = settings(search != 0); S.sweeps = 0; CHECK(refused(c.inputs(search != 0), S, "Jacobi sweeps")); }
    }
    const Call c = make_call(0);
    { GfwRsSettings S = settings(true); S.step_s = 0.0; CHECK(refused(c.inputs(true), S, "step")); }
    { GfwRsSettings S = settings(true); S.step_s = NAN; CHECK(refused(c.inputs(true), S, "step")); }
    { GfwRsSettings S = settings(true); S.radius_s = -1.0; CHECK(refused(c.inputs(true), S, "radius")); }
    { GfwRsSettings S = settings(true); S.radius_s = 1e12; CHECK(refused(c.inputs(true), S, "candidates")); }
    { GfwRsSettings S = settings(true); S.rounds = 9; CHECK(refused(c.inputs(true), S, "9 rounds, 1 .. 8")); }
    { GfwRsSettings S = settings(true); S.initial_delay_s = INFINITY; CHECK(refused(c.inputs(true), S, "initial delay")); }
    { Call x = c; x.cand_first = {0, 4, 3, 7}; CHECK(refused(x.inputs(false), settings(false), "range 1: cand_first descends")); }
    { Call x = c; x.cand_first = {0, 4, 6, 6}; CHECK(refused(x.inputs(false), settings(false), "range 2: cand_first ends at 6, the call has 7 candidates")); }
    { GfwRsInputs I = make_call(0).inputs(false); I.n_ranges = 0; CHECK(gfw_rs_check(I, settings(false), why, sizeof(why))); }      // no ranges: nothing else is looked at
}

static void test_layout_and_fill() {
    for (int search = 0; search < 2; ++search) {
        const int lead = search ? 0 : 6;
        const Call c = make_call(lead);
        const GfwRsInputs I = c.inputs(search != 0);
        const GfwRsLayout L = gfw_rs_layout(I);
        CHECK(L.points == 137 && L.max_pair == 65);
        char *h = (char *)malloc(L.total);                                    // exactly the layout's bytes
        GfwRsArgs A;
        memset(&A, 0, sizeof(A));
        gfw_rs_fill(L, I, h, D, A);
        const int32_t *prange = (const int32_t *)(h + L.o_prange), *pfirst = (const int32_t *)(h + L.o_pfirst);
        const int want_range[5] = {0, 0, 0, 2, 2}, want_first[6] = {0, 0, 1, 65, 130, 137};
        for (int p = 0; p < 5; ++p) CHECK(prange[p] == want_range[p]);
        for (int p = 0; p < 6; ++p) CHECK(pfirst[p] == want_first[p]);       // counted from 0 whatever the caller's first point
        const float *pts = (const float *)(h + L.o_pts);
        CHECK(pts[0] == (float)(lead * 2) && pts[137 * 2] == (float)(lead * 2) + 0.5f && pts[137 * 4 - 1] == (float)((lead + 137) * 2 - 1) + 0.5f);
        const double *tt = (const double *)(h + L.o_tt);
        CHECK(tt[0] == 0.5 && tt[8] == 2.5 && tt[3] == 1250000.0 / 1000000.0);
        CHECK(((const double *)(h + L.o_tq))[8 * 4 + 1] == 0.08 && ((const int64_t *)(h + L.o_pts_us))[9] == 1000000 + 33333 * 5);
        CHECK(A.n_ranges == 3 && A.n_pairs == 5 && A.total == 137 && A.n_track == 9 && A.lds_points == 65);
        CHECK((const char *)A.track_q == D + L.o_tq && (const char *)A.points == D + L.o_pts);
        if (!search) {
            const int64_t *pc = (const int64_t *)(h + L.o_pcfirst);
            const int64_t want_pc[5] = {0, 4, 8, 12, 13};                     // ranges of 4, 2, 1 candidates: 3 pairs x 4, then 2 pairs x 1
            for (int p = 0; p < 5; ++p) CHECK(pc[p] == want_pc[p]);
            CHECK(L.pair_costs == 14 && L.max_cand == 4 && ((const double *)(h + L.o_cand))[6] == 0.006);
            CHECK((const char *)A.pc_first == D + L.o_pcfirst);
        } else CHECK(A.cand_first == nullptr && L.pair_costs == 0);
        free(h);
    }
}

static void test_rounds() {
    CHECK(gfw_rs_round0_count(0.03, 0.003) == 21 && gfw_rs_round0_count(3.0, 0.003) == 2001 && gfw_rs_round0_count(0.0, 0.003) == 1 && gfw_rs_round0_count(0.0029, 0.003) == 1);
    CHECK(gfw_rs_round0_count(1e12, 0.003) == -1);
    const GfwRsSettings S = settings(true);
    GfwRsArgs A;
    memset(&A, 0, sizeof(A));
    double step = 0.003;
    for (int round = 0; round < 4; ++round) {
        gfw_rs_round(S, round, A);
        CHECK(A.mode == (round ? 2 : 1) && A.n_cand == (round ? 17 : 21) && A.at == (round ? 21 + 17 * (round - 1) : 0) && A.total_cand == 21 + 3 * 17);
        CHECK(A.step == step && A.next_step == step / 8.0 && A.half == 10 && A.last == (round == 3));
        step = step / 8.0;
    }
    gfw_rs_constants(1920, 1080, 960, 540, 12.0, S, A);
    CHECK(A.readout_s == 12.0 / 1000.0 && A.flow_h == 540.0 && A.fh == 540.0f && A.vw == 1920.0f && A.hypotheses == 16 && A.refits == 3 && A.sweeps == 8);
}

static void test_lookup() {
    for (int n : {2, 3, 9}) {
        double *T = (double *)malloc(sizeof(double) * n), *Q = (double *)malloc(sizeof(double) * 4 * n);      // exactly the track
        for (int i = 0; i < n; ++i) { T[i] = 1.0 + 0.25 * i; Q[i * 4] = (i & 1) ? -1.0 : 1.0; Q[i * 4 + 1] = 0.1 * i * ((i & 1) ? -1.0 : 1.0); Q[i * 4 + 2] = 0.0; Q[i * 4 + 3] = 0.0; }
        double q[4];
        for (double t : {-5.0, 1.0, 1.1, 1.25, 1.0 + 0.25 * (n - 1), 99.0, (double)NAN}) {
            gfw_rs_quat_at(T, Q, n, t, q);
            if (t == t) CHECK(fabs((((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])) + (q[3] * q[3]) - 1.0) < 1e-15);
        }
        gfw_rs_quat_at(T, Q, n, -5.0, q);
        CHECK(q[0] == 1.0 && q[1] == 0.0);                                    // clamped to the first sample
        gfw_rs_quat_at(T, Q, n, 99.0, q);
        const double s = (n - 1) & 1 ? 1.0 : -1.0, len = sqrt(1.0 + 0.01 * (n - 1) * (n - 1));      // neighbours have opposite signs: the last sample arrives flipped
        CHECK(fabs(q[0] * s - 1.0 / len) < 1e-15 && fabs(q[1] * s - 0.1 * (n - 1) / len) < 1e-15);      // .. and to the last, in the sign the shorter arc gave it
        gfw_rs_quat_at(T, Q, n, 1.125, q);                                    // halfway to a sample of the opposite sign: the flip keeps the short arc
        CHECK(q[0] > 0.99 && q[1] > 0.0);
        free(T); free(Q);
    }
    const double q[4] = {0.0, 1.0, 0.0, 0.0}, p[3] = {0.0, 0.6, 0.8};       // the rotation by pi about X after diag(1, -1, -1): the identity
    double o[3];
    gfw_rs_to_world(q, p, o);
    CHECK(o[0] == 0.0 && o[1] == 0.6 && o[2] == 0.8);
    double G[6] = {2.0, 0.0, 0.0, 1.0, 0.0, 1.0}, t[3];                       // of equal eigenvalues the first index wins
    gfw_rs_smallest(G, 8, t);
    CHECK(t[0] == 0.0 && t[1] == 1.0 && t[2] == 0.0);
}

int main() {
    test_check();
    test_layout_and_fill();
    test_rounds();
    test_lookup();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("rs-sync host code ok\n");
    return 0;
}
