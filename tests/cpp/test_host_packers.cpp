// test_host_packers.cpp — TEST INFRASTRUCTURE: the entry points' host packers (gfw_matrices_host.h, gfw_zoom_host.h, gfw_sync_host.h, gfw_sync_gyro_host.h) in a program
// of their own, built with AddressSanitizer and UBSan (tests/test_cpp_host_packers.py; host pass only, no device, no library).  Every packer fills a heap block of
// EXACTLY its layout's total — one byte more is the sanitizer's — at a fake device base, so that a host pointer handed out as a device pointer shows; checked are the
// alignment of every part, the argument pointers (d + offset) and that the contents come back out.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_matrices.h"
#include "../../gyroflow_amd/csrc/gfw_zoom.h"
#include "../../gyroflow_amd/csrc/gfw_sync.h"
#include "../../gyroflow_amd/csrc/gfw_sync_gyro.h"
#include "../../gyroflow_amd/csrc/gfw_matrices_host.h"
#include "../../gyroflow_amd/csrc/gfw_zoom_host.h"
#include "../../gyroflow_amd/csrc/gfw_sync_host.h"
#include "../../gyroflow_amd/csrc/gfw_sync_gyro_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const char *const D = (const char *)(uintptr_t)0x500000000000ull;     // the "device" side of every block: never dereferenced
struct Block {
    char *h; size_t total;
    explicit Block(size_t n) : h((char *)malloc(n)), total(n) { memset(h, 0xA5, n); }
    ~Block() { free(h); }
    template <class T> const T *at(const void *dev) const {                  // the host bytes behind a device pointer of this block
        const size_t off = (size_t)((const char *)dev - D);
        CHECK(off <= total);
        return (const T *)(h + off);
    }
};
static bool aligned(std::initializer_list<size_t> offs) { for (size_t o : offs) if (o % 8) return false; return true; }

static gfw_frame_stab make_stab(const std::vector<double> &ibis, const std::vector<double> &ois, double height) {
    gfw_frame_stab s;
    memset(&s, 0, sizeof(s));
    s.offset = 12.5; s.sensor_size[0] = 6000; s.sensor_size[1] = 3376;
    s.crop_area[0] = 120; s.crop_area[1] = 338; s.crop_area[2] = 5760; s.crop_area[3] = 2700;
    s.pixel_pitch[0] = 3; s.pixel_pitch[1] = 4; s.width = 320; s.height = height;
    s.ibis_count = (int)ibis.size() / 4; s.ois_count = (int)ois.size() / 4;
    s.ibis = ibis.empty() ? nullptr : ibis.data(); s.ois = ois.empty() ? nullptr : ois.data();
    return s;
}
static std::vector<double> ramp(size_t n, double from) { std::vector<double> v(n); for (size_t i = 0; i < n; ++i) v[i] = from + (double)i; return v; }

// a table's entries against the ABI structs they were made of; `o_points`: where the control points start
static void check_stab_table(const Block &B, const GfwStab *d_table, const gfw_frame_stab *const *stabs, const double *y_signs, int n, size_t o_points) {
    const GfwStab *t = B.at<GfwStab>(d_table);
    size_t at = o_points;
    for (int i = 0; i < n; ++i) {
        if (!stabs[i]) { CHECK(t[i].ibis_n == -1 && t[i].ois_n == -1 && !t[i].ibis && !t[i].ois); continue; }
        const gfw_frame_stab &s = *stabs[i];
        CHECK(t[i].ibis_n == s.ibis_count && t[i].ois_n == s.ois_count);
        CHECK((const char *)t[i].ibis == D + at && (const char *)t[i].ois == D + at + 32 * (size_t)s.ibis_count);
        CHECK(!s.ibis_count || !memcmp(B.h + at, s.ibis, 32 * (size_t)s.ibis_count));
        CHECK(!s.ois_count || !memcmp(B.h + at + 32 * (size_t)s.ibis_count, s.ois, 32 * (size_t)s.ois_count));
        CHECK(t[i].offset == s.offset && t[i].sensor_h == s.sensor_size[1] && t[i].crop_y == s.crop_area[1] && t[i].crop_h == s.crop_area[3] && t[i].height == s.height);
        CHECK(t[i].scale_x == s.width / s.crop_area[2] / s.pixel_pitch[0]);
        CHECK(t[i].scale_y == s.height / s.crop_area[3] / s.pixel_pitch[1] * y_signs[i]);
        at += stab_point_bytes(&s);
    }
    CHECK(at <= B.total);
}

static void test_matrices() {
    const std::vector<double> ib = ramp(12, 1.0), oi = ramp(4, 100.0), oi2 = ramp(8, 200.0);
    const gfw_frame_stab s0 = make_stab(ib, oi, 180), s2 = make_stab({}, oi2, 180);              // s2: 0 IBIS and 2 OIS points
    const gfw_frame_stab *stabs[3] = {&s0, nullptr, &s2};
    gfw_frame_timing t[3];
    memset(t, 0, sizeof(t));
    t[2].framebuffer_inverted = 1;
    const double signs[3] = {1.0, 1.0, -1.0};
    BlockLayout L;
    const size_t pts = gfw_stab_points_total(stabs, 3);
    CHECK(pts == 32 * (3 + 1 + 2));
    const GfwStabTable S = gfw_stab_table_layout(L, 3, pts);
    CHECK(aligned({S.o_table, S.o_points, L.total}) && L.total == sizeof(GfwStab) * 3 + pts);
    Block B(L.total);
    const GfwStab *d = gfw_stab_table_fill(S, stabs, t, 3, B.h, D);
    CHECK((const char *)d == D + S.o_table);
    check_stab_table(B, d, stabs, signs, 3, S.o_points);
}

static gfw_zoom_frame make_frame(int k) {
    gfw_zoom_frame f;
    memset(&f, 0, sizeof(f));
    f.timestamp_ms = 100.0 + k; f.fov = 1.0 + 0.01 * k; f.lens_correction_amount = 1.0;
    for (int i = 0; i < 9; ++i) f.new_k[i] = k * 10 + i;
    return f;
}
static void test_zoom() {
    // 1 frame and 3 frames with caller rotations: 36 and 108 bytes, neither a multiple of 8
    for (int n : {1, 3}) {
        std::vector<gfw_zoom_frame> frames;
        for (int k = 0; k < n; ++k) frames.push_back(make_frame(k));
        std::vector<float> rot((size_t)n * 9);
        for (size_t i = 0; i < rot.size(); ++i) rot[i] = (float)i * 0.5f;
        const std::vector<double> ib = ramp(12, 1.0), oi = ramp(4, 100.0), oi2 = ramp(8, 200.0);
        const gfw_frame_stab s0 = make_stab(ib, oi, 180), s2 = make_stab({}, oi2, 180);
        const gfw_frame_stab *stabs[3] = {&s0, nullptr, &s2};                                    // (n = 1: the first entry alone)
        const double signs[3] = {1.0, 1.0, 1.0};                                                // at_timestamp_for_points: no framebuffer sign
        const size_t pts = gfw_stab_points_total(stabs, n);
        const GfwZoomLayout Z = gfw_zoom_layout(n, true, true, pts, false, 0);
        CHECK(aligned({Z.o_frames, Z.o_rot, Z.stab.o_table, Z.stab.o_points, Z.o_ref, Z.o_mesh, Z.total}));
        CHECK(Z.stab.o_table - Z.o_rot == ((size_t)n * 36 + 7) / 8 * 8 && Z.total == Z.stab.o_points + pts);
        Block B(Z.total);
        GfwZoomArgs A;
        memset(&A, 0xff, sizeof(A));
        gfw_zoom_fill(Z, frames.data(), n, rot.data(), stabs, nullptr, nullptr, B.h, D, A);
        CHECK((const char *)A.frames == D + Z.o_frames && (const char *)A.rotations == D + Z.o_rot && (const char *)A.stabs == D + Z.stab.o_table);
        CHECK(!A.mesh_ref && !A.mesh_data);
        CHECK(!memcmp(B.at<char>(A.frames), frames.data(), sizeof(gfw_zoom_frame) * n) && !memcmp(B.at<char>(A.rotations), rot.data(), 36 * (size_t)n));
        check_stab_table(B, A.stabs, stabs, signs, n, Z.stab.o_points);
    }
    // meshes [A, A, none, B] without rotations or stabiliser data: one copy of A, a zero reference, B behind A
    {
        std::vector<gfw_zoom_frame> frames;
        for (int k = 0; k < 4; ++k) frames.push_back(make_frame(k));
        const std::vector<double> a = ramp(11, 1000.0), b = ramp(5, 2000.0);
        const double *meshes[4] = {a.data(), a.data(), nullptr, b.data()};
        const size_t lens[4] = {11, 11, 0, 5};
        CHECK(gfw_zoom_mesh_doubles(meshes, lens, 4) == 16);
        const GfwZoomLayout Z = gfw_zoom_layout(4, false, false, 0, true, 16);
        CHECK(aligned({Z.o_frames, Z.o_rot, Z.stab.o_table, Z.stab.o_points, Z.o_ref, Z.o_mesh, Z.total}) && Z.total == sizeof(gfw_zoom_frame) * 4 + 8 * 4 + 8 * 16);
        Block B(Z.total);
        GfwZoomArgs A;
        memset(&A, 0xff, sizeof(A));
        gfw_zoom_fill(Z, frames.data(), 4, nullptr, nullptr, meshes, lens, B.h, D, A);
        CHECK(!A.rotations && !A.stabs && (const char *)A.mesh_ref == D + Z.o_ref && (const char *)A.mesh_data == D + Z.o_mesh);
        const int32_t *ref = B.at<int32_t>(A.mesh_ref);
        const int32_t want[8] = {0, 11, 0, 11, 0, 0, 11, 5};
        CHECK(!memcmp(ref, want, sizeof(want)));
        const double *m = B.at<double>(A.mesh_data);
        CHECK(!memcmp(m, a.data(), 88) && !memcmp(m + 11, b.data(), 40));
    }
    // FovIterative::new, once
    {
        const gfw_zoom_search s = {320, 180, 240, 135, 0.25f, 1};
        GfwZoomArgs A;
        gfw_zoom_search_args(s, A);
        const float ratio = 320.0f / 240.0f;
        CHECK(A.w == 320.0f && A.h == 180.0f && A.margin == 0.25f && A.horizontal == 1 && A.readout_dim == 320);
        CHECK(A.out_dim0 == 240.0f * ratio && A.inv_aspect == (135.0f * ratio) / (240.0f * ratio));
    }
}

static void test_sync() {
    const int64_t ts[4] = {1000, 2000, 3000, 4000};
    const int32_t first[3] = {0, 0, 3};                                                        // 2 pairs with 0 and 3 points: 12 bytes of firsts, padded
    const float pa[6] = {1, 2, 3, 4, 5, 6}, pb[6] = {7, 8, 9, 10, 11, 12};
    const double cand[4] = {-1.5, 8.0, 2.5, 9.0};
    // 0 pairs, caller candidates
    {
        const GfwSyncLayout S = gfw_sync_layout(0, 0, 2);
        CHECK(aligned({S.o_ts, S.o_first, S.o_pts, S.o_cand, S.total}) && S.total == 8 + 32);
        Block B(S.total);
        GfwSyncArgs A;
        memset(&A, 0, sizeof(A));
        gfw_sync_fill(S, nullptr, nullptr, nullptr, nullptr, 0, cand, 2, -1, 0, 0, 0, B.h, D, A);
        CHECK((const char *)A.pair_first == D + S.o_first && (const char *)A.candidates == D + S.o_cand && A.n_pairs == 0 && A.total == 0);
        CHECK(*B.at<int32_t>(A.pair_first) == 0 && !memcmp(B.at<char>(A.candidates), cand, 32));
    }
    // 2 pairs, caller candidates
    {
        const GfwSyncLayout S = gfw_sync_layout(2, 3, 2);
        CHECK(aligned({S.o_ts, S.o_first, S.o_pts, S.o_cand, S.total}) && S.o_pts - S.o_first == 16 && S.total == 32 + 16 + 48 + 32);
        Block B(S.total);
        GfwSyncArgs A;
        memset(&A, 0, sizeof(A));
        gfw_sync_fill(S, ts, first, pa, pb, 2, cand, 2, -1, 0, 0, 0, B.h, D, A);
        CHECK((const char *)A.pair_ts == D + S.o_ts && (const char *)A.pair_first == D + S.o_first && (const char *)A.points == D + S.o_pts && (const char *)A.candidates == D + S.o_cand);
        CHECK(A.n_pairs == 2 && A.total == 3);
        CHECK(!memcmp(B.at<char>(A.pair_ts), ts, 32) && !memcmp(B.at<char>(A.pair_first), first, 12));
        CHECK(!memcmp(B.at<char>(A.points), pa, 24) && !memcmp(B.at<char>(A.points) + 24, pb, 24) && !memcmp(B.at<char>(A.candidates), cand, 32));
    }
    // mode 0 with 0 and with 5 coarse candidates (`search_size as usize`), mode 1 at 30 fps (`-33..33`)
    CHECK(gfw_sync_coarse_steps(0, 0.9, 30.0) == 0.0 && gfw_sync_coarse_steps(0, -3.0, 30.0) == 0.0 && gfw_sync_coarse_steps(0, (double)NAN, 30.0) == 0.0);
    CHECK(gfw_sync_coarse_steps(0, 5.9, 30.0) == 5.0 && gfw_sync_coarse_steps(1, 5.9, 30.0) == 33.0);
    for (int n : {0, 5}) {
        const GfwSyncLayout S = gfw_sync_layout(2, 3, (size_t)n);
        CHECK(S.total == 32 + 16 + 48 + 16 * (size_t)n);
        Block B(S.total);
        GfwSyncArgs A;
        memset(&A, 0, sizeof(A));
        gfw_sync_fill(S, ts, first, pa, pb, 2, nullptr, n, 0, 40.0, 5.9, 12.0, B.h, D, A);
        const double *c = B.at<double>(A.candidates);
        for (int i = 0; i < n; ++i) CHECK(c[i * 2] == 40.0 + (-(5.9 / 2.0) + (double)i) && c[i * 2 + 1] == 12.0);
    }
    {
        const GfwSyncLayout S = gfw_sync_layout(2, 3, 66);
        Block B(S.total);
        GfwSyncArgs A;
        memset(&A, 0, sizeof(A));
        gfw_sync_fill(S, ts, first, pa, pb, 2, nullptr, 66, 1, 40.0, 5.9, 12.0, B.h, D, A);
        const double *c = B.at<double>(A.candidates);
        for (int i = 0; i < 66; ++i) CHECK(c[i * 2] == 0.0 && c[i * 2 + 1] == (double)(i - 33));
    }
}

static void test_gyro() {
    // two ranges behind a lead-in on all three series (first[0] > 0); the second range is empty.  Range 0's gyro slice: not ascending, one duplicated key (the later sample wins)
    const int32_t ef[3] = {2, 5, 5}, gf[3] = {1, 6, 6}, cf[3] = {3, 7, 7};
    std::vector<double> est = ramp(5 * 4, 0.0), gyro(6 * 4), cand = ramp(7, 50.0);
    const uint8_t est_has[5] = {1, 1, 1, 0, 1}, gyro_has[6] = {1, 1, 1, 1, 0, 1};
    const double gts[6] = {-1.0, 3.0, 1.0, 2.0, 1.0, 4.0};                                     // keys of entries 1..5: 3000, 1000, 2000, 1000 (again), 4000
    for (int i = 0; i < 6; ++i) { gyro[i * 4] = gts[i]; for (int a = 1; a < 4; ++a) gyro[i * 4 + a] = i * 10 + a; }
    const GfwGyroSeries se = {ef, est.data(), est_has}, sg = {gf, gyro.data(), gyro_has};
    {
        const GfwGyroLayout L = gfw_gyro_layout(2, 3, 5, 4);
        CHECK(aligned({L.o_ranges, L.o_est, L.o_has, L.o_keys, L.o_val, L.o_cand, L.total}) && L.o_keys - L.o_has == 8);
        CHECK(L.total == sizeof(GfwGyroRange) * 2 + 96 + 8 + 40 + 160 + 32);
        Block B(L.total);
        GfwGyroArgs A;
        memset(&A, 0, sizeof(A));
        const int max_cand = gfw_gyro_fill(L, se, sg, 2, cf, cand.data(), 0, 0.0, 0.0, B.h, D, A);
        CHECK(max_cand == 4);
        CHECK((const char *)A.ranges == D + L.o_ranges && (const char *)A.est == D + L.o_est && (const char *)A.est_has == D + L.o_has);
        CHECK((const char *)A.keys == D + L.o_keys && (const char *)A.gyro == D + L.o_val && (const char *)A.candidates == D + L.o_cand);
        const GfwGyroRange *r = B.at<GfwGyroRange>(A.ranges);
        CHECK(r[0].est_first == 0 && r[0].est_n == 3 && r[0].gyro_first == 0 && r[0].gyro_n == 4 && r[0].cand_first == 0 && r[0].cand_n == 4);
        CHECK(r[1].est_first == 3 && r[1].est_n == 0 && r[1].gyro_first == 4 && r[1].gyro_n == 0 && r[1].cand_first == 4 && r[1].cand_n == 0);
        CHECK(!memcmp(B.at<char>(A.est), est.data() + 2 * 4, 96));
        const uint8_t *has = B.at<uint8_t>(A.est_has);
        CHECK(has[0] == 1 && has[1] == 0 && has[2] == 1);
        const unsigned long long *keys = B.at<unsigned long long>(A.keys);
        CHECK(keys[0] == 1000 && keys[1] == 2000 && keys[2] == 3000 && keys[3] == 4000);
        const double *v = B.at<double>(A.gyro);
        CHECK(v[0] == 41 && v[1] == 42 && v[2] == 43 && v[3] == 0.0);                           // key 1000: entry 4 (the later one), which has no gyro
        CHECK(v[4] == 31 && v[7] == 1.0 && v[8] == 11 && v[11] == 1.0 && v[12] == 51 && v[15] == 1.0);
        CHECK(!memcmp(B.at<char>(A.candidates), cand.data() + 3, 32));
    }
    // the search's own candidates: 4 per range, the empty range's too
    {
        const GfwGyroLayout L = gfw_gyro_layout(2, 3, 5, 8);
        Block B(L.total);
        GfwGyroArgs A;
        memset(&A, 0, sizeof(A));
        const int max_cand = gfw_gyro_fill(L, se, sg, 2, nullptr, nullptr, 4, 10.0, 2.5, B.h, D, A);
        CHECK(max_cand == 4);
        const GfwGyroRange *r = B.at<GfwGyroRange>(A.ranges);
        CHECK(r[0].cand_first == 0 && r[0].cand_n == 4 && r[1].cand_first == 4 && r[1].cand_n == 4);
        const double *c = B.at<double>(A.candidates);
        for (int i = 0; i < 8; ++i) CHECK(c[i] == 10.0 - 2.5 + (double)(i % 4));
    }
}

int main() {
    test_matrices();
    test_zoom();
    test_sync();
    test_gyro();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("host packers ok\n");
    return 0;
}
