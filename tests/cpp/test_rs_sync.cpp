// C++ use of gyroflow::find_offsets_rssync (include/gfwarp.hpp): the rs-sync offset search of a clip's ranges, against the numpy statement's stored results
// (tests/golden/rs_sync_cpp.txt, written by tests/test_cpp_rs_sync.py's generator; numbers as C hex floats, so nothing is rounded on the way).
//
//   test_rs_sync validate <fixture>   ranges that reach no search need no context, ranges that do fail loudly without one; the readout rules; needs no GPU
//   test_rs_sync search <fixture>     find_offsets_rssync on the device: timestamps, offsets and costs of every run equal to the statement's to the bit
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "gfwarp.hpp"

using namespace gyroflow;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

struct Run { SyncParams sync; std::vector<std::tuple<double, double, double>> want; };
struct Fixture {
    KernelParams kp;
    int model = 0, digital = 0;
    gfw_sync_rs_cfg cfg;
    std::vector<int64_t> track_ts;
    std::vector<double> track_q;
    std::vector<std::pair<int64_t, int64_t>> ranges;
    std::vector<MatchedPoints> matched;
    std::vector<Run> runs;
};
static double num(std::ifstream &f) { std::string s; CHECK(static_cast<bool>(f >> s)); return std::strtod(s.c_str(), nullptr); }
static long long integer(std::ifstream &f) { long long v = 0; CHECK(static_cast<bool>(f >> v)); return v; }
static Fixture load(const char *path) {
    std::ifstream f(path);
    CHECK(f.good());
    Fixture d;
    std::string hex;
    CHECK(static_cast<bool>(f >> hex) && hex.size() == 2 * sizeof(KernelParams));
    for (size_t i = 0; i < sizeof(KernelParams); ++i) ((unsigned char *)&d.kp)[i] = (unsigned char)std::strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    d.model = (int)integer(f); d.digital = (int)integer(f);
    std::memset(&d.cfg, 0, sizeof(d.cfg));
    d.cfg.video_width = (int32_t)integer(f); d.cfg.video_height = (int32_t)integer(f); d.cfg.flow_width = (int32_t)integer(f); d.cfg.flow_height = (int32_t)integer(f);
    d.cfg.rounds = (int32_t)integer(f); d.cfg.refine = (int32_t)integer(f); d.cfg.hypotheses = (int32_t)integer(f); d.cfg.refits = (int32_t)integer(f);
    d.cfg.jacobi_sweeps = (int32_t)integer(f);
    d.cfg.frame_readout_time_ms = num(f); d.cfg.step_s = num(f); d.cfg.loss_scale = num(f);
    for (int i = 0; i < 9; ++i) d.cfg.camera_matrix[i] = num(f);
    for (long long n = integer(f); n > 0; --n) { d.track_ts.push_back(integer(f)); for (int i = 0; i < 4; ++i) d.track_q.push_back(num(f)); }
    for (long long n = integer(f); n > 0; --n) { const long long a = integer(f), b = integer(f); d.ranges.emplace_back(a, b); }
    for (long long n = integer(f); n > 0; --n) {
        MatchedPoints m;
        m.timestamp_us = integer(f); m.next_timestamp_us = integer(f);
        for (long long k = integer(f); k > 0; --k) { const float ax = (float)num(f), ay = (float)num(f), bx = (float)num(f), by = (float)num(f); m.points.emplace_back(ax, ay); m.next_points.emplace_back(bx, by); }
        d.matched.push_back(m);
    }
    for (long long n = integer(f); n > 0; --n) {
        Run r;
        r.sync.initial_offset = num(f); r.sync.search_size = num(f);
        for (long long k = integer(f); k > 0; --k) { const double t = num(f), o = num(f), c = num(f); r.want.emplace_back(t, o, c); }
        d.runs.push_back(r);
    }
    return d;
}

static int run_validate(const Fixture &d) {
    CHECK(rs_readout_time_ms(0.0, 30.0, false) == 1000.0 / 30.0 / 2.0 && rs_readout_time_ms(12.0, 30.0, false) == 12.0 && rs_readout_time_ms(12.0, 30.0, true) == 0.01);
    const SyncParams sp = d.runs[0].sync;
    std::vector<std::pair<int64_t, int64_t>> none = {{5, 5}, {9, 3}, {d.matched[0].timestamp_us, d.matched[0].timestamp_us + 1}};      // empty, reversed, one pair: no search
    CHECK(find_offsets_rssync(nullptr, d.kp, d.cfg, none, d.matched, sp, d.track_ts, d.track_q).empty());
    try { find_offsets_rssync(nullptr, d.kp, d.cfg, d.ranges, d.matched, sp, d.track_ts, d.track_q); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("rs-sync") != std::string::npos); }
    std::vector<MatchedPoints> odd = d.matched;
    odd[1].next_points.pop_back();
    try { find_offsets_rssync(nullptr, d.kp, d.cfg, d.ranges, odd, sp, d.track_ts, d.track_q); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("one length") != std::string::npos); }
    std::vector<double> q = d.track_q;
    q.pop_back();
    try { find_offsets_rssync(nullptr, d.kp, d.cfg, d.ranges, d.matched, sp, d.track_ts, q); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("per track timestamp") != std::string::npos); }
    std::printf("validate ok: %zu ranges, %zu pairs, %zu runs\n", d.ranges.size(), d.matched.size(), d.runs.size());
    return 0;
}

static int run_search(const Fixture &d) {
    const int W = 64, H = 32;
    std::vector<uint8_t> src((size_t)W * H), dst((size_t)W * H);
    KernelParams cp = d.kp;
    cp.width = cp.output_width = W; cp.height = cp.output_height = H; cp.stride = cp.output_stride = W;
    cp.bytes_per_pixel = 1; cp.pix_element_count = 1; cp.interpolation = 2; cp.matrix_count = 1; cp.max_pixel_value = cp.pixel_value_limit = 255.0f;
    Buffers b;
    b.input.size = {W, H, W}; b.input.data = BufferSource::cpu(src.data(), src.size());
    b.output.size = {W, H, W}; b.output.data = BufferSource::cpu(dst.data(), dst.size());
    const gfw_buffers ab = b.to_abi();
    gfw_ctx *ctx = gfw_create(&cp, Luma8::ID, d.model, d.digital, &ab, 0);
    CHECK(ctx != nullptr);
    size_t accepted = 0, refused = 0;
    for (const Run &r : d.runs) {
        const auto got = find_offsets_rssync(ctx, d.kp, d.cfg, d.ranges, d.matched, r.sync, d.track_ts, d.track_q);
        CHECK(std::string(gfw_last_backend(ctx)) == "sync_rs_search");
        CHECK(got.size() == r.want.size());
        for (size_t i = 0; i < got.size(); ++i) {
            const double g[3] = {std::get<0>(got[i]), std::get<1>(got[i]), std::get<2>(got[i])}, w[3] = {std::get<0>(r.want[i]), std::get<1>(r.want[i]), std::get<2>(r.want[i])};
            CHECK(std::memcmp(g, w, sizeof(g)) == 0);
        }
        accepted += got.size();
        refused += got.empty();
    }
    CHECK(accepted > 0 && refused > 0);
    std::printf("search ok: %zu runs, %zu offsets\n", d.runs.size(), accepted);
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::string(argv[1]) == "validate") return run_validate(load(argv[2]));
    if (argc >= 3 && std::string(argv[1]) == "search") return run_search(load(argv[2]));
    std::printf("usage: test_rs_sync validate | search <fixture>\n");
    return 2;
}
