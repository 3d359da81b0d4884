// C++ use of gyroflow::find_offsets_visual (include/gfwarp.hpp): the visual-features offset / readout-time search of a clip's ranges.
//
//   test_sync validate   no ranges, the loud failure without a context; needs no GPU
//   test_sync search     a fisheye range of three pairs over a synthetic gyro track on the device: the search's value and cost equal the last minimum of
//                        gfw_sync_visual_costs over the same coarse and fine candidates, the middle timestamp and the 90 % rule are applied, for_rs searches
//                        the readout time, a range without matched pairs still answers (every cost 0: the last candidate)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gfwarp.hpp"

using namespace gyroflow;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static const int W = 320, H = 180;

static KernelParams points_params() {
    KernelParams p;
    std::memset(&p, 0, sizeof(p));
    p.width = p.output_width = W; p.height = p.output_height = H;
    p.f[0] = p.f[1] = 0.47f * W; p.c[0] = W / 2.0f; p.c[1] = H / 2.0f;
    p.k[0] = 0.045f; p.k[1] = 0.02f; p.k[2] = -0.02f; p.k[3] = 0.006f;
    p.input_vertical_stretch = 1.0f; p.input_horizontal_stretch = 1.0f; p.light_refraction_coefficient = 1.0f; p.lens_correction_amount = 1.0f; p.fov = 1.0f;
    return p;
}
static gfw_sync_search sync_search() {
    gfw_sync_search s;
    std::memset(&s, 0, sizeof(s));
    s.width = W; s.height = H;
    s.new_k[0] = s.new_k[4] = 0.47 * W; s.new_k[2] = W / 2.0; s.new_k[5] = H / 2.0; s.new_k[8] = 1.0;
    return s;
}
static std::vector<MatchedPoints> matches() {
    std::vector<MatchedPoints> out;
    unsigned seed = 12345u;
    auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)((seed >> 8) & 0xffff) / 65536.0f; };
    const int sizes[4] = {40, 0, 70, 130};
    for (int k = 0; k < 4; ++k) {
        MatchedPoints m;
        m.timestamp_us = 1200000 + 300000 * k; m.next_timestamp_us = m.timestamp_us + 66667;
        for (int i = 0; i < sizes[k]; ++i) {
            const float x = 40.0f + 240.0f * next(), y = 30.0f + 120.0f * next();
            m.points.emplace_back(x, y);
            m.next_points.emplace_back(x + 6.0f * (next() - 0.5f), y + 6.0f * (next() - 0.5f));
        }
        out.push_back(m);
    }
    return out;
}

static int run_validate() {
    const KernelParams p = points_params();
    CHECK(find_offsets_visual(nullptr, p, sync_search(), {}, matches(), SyncParams{0.0, 10.0}, 0.0, 30.0).empty());
    try { find_offsets_visual(nullptr, p, sync_search(), {{1000000, 2000000}}, matches(), SyncParams{0.0, 10.0}, 0.0, 30.0); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("sync") != std::string::npos); }
    std::printf("validate ok\n");
    return 0;
}

// the last minimum of gfw_sync_visual_costs over `cand`: what `reduce_with(find_min)` returns
static size_t last_minimum(gfw_ctx *ctx, const KernelParams &p, const gfw_sync_search &s, const std::vector<MatchedPoints> &ms, const std::vector<double> &cand, double *cost) {
    std::vector<int64_t> ts; std::vector<int32_t> first{0}; std::vector<float> a, b;
    for (const MatchedPoints &m : ms) {
        if (m.points.empty()) continue;
        ts.push_back(m.timestamp_us); ts.push_back(m.next_timestamp_us);
        for (const auto &pt : m.points) { a.push_back(pt.first); a.push_back(pt.second); }
        for (const auto &pt : m.next_points) { b.push_back(pt.first); b.push_back(pt.second); }
        first.push_back((int32_t)(a.size() / 2));
    }
    std::vector<double> costs(cand.size() / 2);
    CHECK(gfw_sync_visual_costs(ctx, &p, &s, ts.data(), first.data(), a.data(), b.data(), (int)(ts.size() / 2), cand.data(), (int)costs.size(), costs.data(), nullptr, 0) == GFW_OK);
    size_t best = 0;
    for (size_t i = 1; i < costs.size(); ++i) if (!(costs[best] < costs[i])) best = i;
    *cost = costs[best];
    return best;
}

static int run_search() {
    KernelParams p = points_params();
    std::vector<uint8_t> src((size_t)W * H), dst((size_t)W * H);
    Buffers b;
    b.input.size = {W, H, W}; b.input.data = BufferSource::cpu(src.data(), src.size());
    b.output.size = {W, H, W}; b.output.data = BufferSource::cpu(dst.data(), dst.size());
    KernelParams cp = p;
    cp.stride = cp.output_stride = W; cp.bytes_per_pixel = 1; cp.pix_element_count = 1; cp.interpolation = 2; cp.matrix_count = 1;
    cp.max_pixel_value = cp.pixel_value_limit = 255.0f;
    const gfw_buffers ab = b.to_abi();
    gfw_ctx *ctx = gfw_create(&cp, Luma8::ID, GFW_MODEL_OPENCV_FISHEYE, GFW_MODEL_NONE, &ab, 0);
    CHECK(ctx != nullptr);
    const int n = 3000;                                                     // 1 kHz, 0.5 .. 3.5 s: a yaw / pitch wobble; the stored smoothed track is the original one
    std::vector<int64_t> tts((size_t)n); std::vector<double> q((size_t)n * 4);
    for (int i = 0; i < n; ++i) {
        const double t = 0.5 + i / 1000.0, yaw = 0.5 * std::sin(7.0 * t), pitch = 0.3 * std::sin(11.0 * t + 1.0);
        const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2), cx = std::cos(pitch / 2), sx = std::sin(pitch / 2);
        tts[(size_t)i] = 500000 + 1000 * (int64_t)i;
        q[(size_t)i * 4] = cy * cx; q[(size_t)i * 4 + 1] = cy * sx; q[(size_t)i * 4 + 2] = sy * cx; q[(size_t)i * 4 + 3] = -sy * sx;
    }
    CHECK(gfw_set_quaternion_tracks(ctx, tts.data(), q.data(), n, tts.data(), q.data(), n) == GFW_OK);
    const std::vector<MatchedPoints> ms = matches();
    const gfw_sync_search s = sync_search();
    const SyncParams sp{3.0, 12.0};
    const auto found = find_offsets_visual(ctx, p, s, {{1000000, 2500000}, {5000000, 6000000}}, ms, sp, 8.0, 30.0);
    CHECK(std::string(gfw_last_backend(ctx)) == "sync_visual_search");
    CHECK(found.size() == 2);
    std::vector<double> cand;
    for (int i = 0; i < 12; ++i) { cand.push_back(sp.initial_offset + (-(sp.search_size / 2.0) + (double)i)); cand.push_back(8.0); }
    double cost = 0.0;
    const double coarse = cand[last_minimum(ctx, p, s, ms, cand, &cost) * 2];
    cand.clear();
    for (int i = 0; i < 200; ++i) { cand.push_back(coarse - 1.0 + ((double)i * 0.01)); cand.push_back(8.0); }
    const double fine = cand[last_minimum(ctx, p, s, ms, cand, &cost) * 2];
    CHECK(std::get<0>(found[0]) == 1750.0 && std::get<1>(found[0]) == fine && std::get<2>(found[0]) == cost && cost > 0.0);
    // the second range has no matched pairs: every cost is 0, the last candidate of either stage wins
    CHECK(std::get<0>(found[1]) == 5500.0 && std::get<1>(found[1]) == (3.0 + (-6.0 + 11.0)) - 1.0 + (199.0 * 0.01) && std::get<2>(found[1]) == 0.0);
    // a search of one coarse candidate (`1.0 as usize`): 2.5, the fine stage ends at 3.49 — inside 90 % of the search size (:137); no candidates, no entry
    const auto tiny = find_offsets_visual(ctx, p, s, {{5000000, 6000000}}, ms, SyncParams{3.0, 1.0}, 8.0, 30.0);
    CHECK(tiny.size() == 1 && std::get<1>(tiny[0]) == 2.5 - 1.0 + (199.0 * 0.01));
    CHECK(find_offsets_visual(ctx, p, s, {{5000000, 6000000}}, ms, SyncParams{3.0, 0.5}, 8.0, 30.0).empty());           // `0.5 as usize` = 0 candidates
    const auto rs = find_offsets_visual(ctx, p, s, {{1000000, 2500000}}, ms, sp, 8.0, 100.0, true);                     // -10 .. 9 ms, then 200 fine ones
    cand.clear();
    for (int i = -10; i < 10; ++i) { cand.push_back(0.0); cand.push_back((double)i); }
    const double rs_coarse = cand[last_minimum(ctx, p, s, ms, cand, &cost) * 2 + 1];
    cand.clear();
    for (int i = 0; i < 200; ++i) { cand.push_back(0.0); cand.push_back(rs_coarse - 1.0 + ((double)i * 0.01)); }
    const double rs_fine = cand[last_minimum(ctx, p, s, ms, cand, &cost) * 2 + 1];
    CHECK(rs.size() == 1 && std::get<0>(rs[0]) == 0.0 && std::get<1>(rs[0]) == rs_fine && std::get<2>(rs[0]) == cost);
    std::printf("search ok: offset %.2f ms (cost %.0f), readout %.2f ms\n", std::get<1>(found[0]), std::get<2>(found[0]), std::get<1>(rs[0]));
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "validate") return run_validate();
    if (argc >= 2 && std::string(argv[1]) == "search") return run_search();
    std::printf("usage: test_sync validate | search\n");
    return 2;
}
