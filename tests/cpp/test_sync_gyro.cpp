// C++ use of gyroflow::find_offsets_essential / initial_offset_fast (include/gfwarp.hpp): the gyro-match offset search of a clip's ranges, against a dump of the
// numpy statement's results for a planted clip (tests/test_cpp_sync_gyro.py writes it; numbers as C hex floats, so nothing is rounded on the way).
//
//   test_sync_gyro validate <dump>   the guards, the loud failure without a context, the median rule, and the host half — range cut, gyro window, max-angle
//                                    skip, the two low-pass calls — equal to the statement's staged ranges to the bit; needs no GPU
//   test_sync_gyro search <dump>     find_offsets_essential and initial_offset_fast on the device: equal to the statement's to the bit
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "gfwarp.hpp"

using namespace gyroflow;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

struct Dump {
    double duration_ms = 0.0, fps = 0.0;
    SyncParams sp;
    std::map<int64_t, TimeIMU> estimated_gyro;
    std::vector<TimeIMU> raw_imu;
    std::vector<std::pair<int64_t, int64_t>> ranges;
    EssentialRanges live;                                                     // the statement's
    std::vector<std::tuple<double, double, double>> offsets;
    SyncParams fast;
};
static double num(std::ifstream &f) { std::string s; CHECK(static_cast<bool>(f >> s)); return std::strtod(s.c_str(), nullptr); }
static long long integer(std::ifstream &f) { long long v = 0; CHECK(static_cast<bool>(f >> v)); return v; }
static TimeIMU imu(std::ifstream &f) { TimeIMU x; x.timestamp_ms = num(f); x.has_gyro = integer(f) != 0; for (int a = 0; a < 3; ++a) x.gyro[a] = num(f); return x; }
static Dump load(const char *path) {
    std::ifstream f(path);
    CHECK(f.good());
    Dump d;
    d.duration_ms = num(f); d.fps = num(f); d.sp.initial_offset = num(f); d.sp.search_size = num(f);
    for (long long n = integer(f); n > 0; --n) { const int64_t key = integer(f); d.estimated_gyro[key] = imu(f); }
    for (long long n = integer(f); n > 0; --n) d.raw_imu.push_back(imu(f));
    for (long long n = integer(f); n > 0; --n) { const int64_t a = integer(f), b = integer(f); d.ranges.emplace_back(a, b); }
    for (long long n = integer(f); n > 0; --n) {
        d.live.index.push_back((size_t)integer(f));
        for (int side = 0; side < 2; ++side) {
            std::vector<double> &rows = side ? d.live.gyro : d.live.est;
            std::vector<uint8_t> &has = side ? d.live.gyro_has : d.live.est_has;
            for (long long m = integer(f); m > 0; --m) { for (int k = 0; k < 4; ++k) rows.push_back(num(f)); has.push_back((uint8_t)integer(f)); }
            (side ? d.live.gyro_first : d.live.est_first).push_back((int32_t)has.size());
        }
    }
    for (long long n = integer(f); n > 0; --n) { const double a = num(f), b = num(f), c = num(f); d.offsets.emplace_back(a, b, c); }
    d.fast.initial_offset = num(f); d.fast.search_size = num(f);
    return d;
}
static bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

static int run_validate(const Dump &d) {
    // :22 and :26 — nothing reaches the device, so no context is needed
    CHECK(find_offsets_essential(nullptr, {}, d.raw_imu, d.duration_ms, d.fps, d.ranges, d.sp).empty());
    CHECK(find_offsets_essential(nullptr, d.estimated_gyro, {}, d.duration_ms, d.fps, d.ranges, d.sp).empty());
    CHECK(find_offsets_essential(nullptr, d.estimated_gyro, d.raw_imu, 0.0, d.fps, d.ranges, d.sp).empty());
    CHECK(find_offsets_essential(nullptr, d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, {}, d.sp).empty());
    CHECK(find_offsets_essential(nullptr, d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, {{5, 5}, {9, 3}}, d.sp).empty());
    const SyncParams same_sp = initial_offset_fast(nullptr, d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, {}, d.sp);
    CHECK(same_sp.initial_offset == d.sp.initial_offset && same_sp.search_size == d.sp.search_size);
    try { find_offsets_essential(nullptr, d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, d.ranges, d.sp); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("sync") != std::string::npos); }
    CHECK(median_offset({3.0}) == 3.0 && median_offset({5.0, 1.0, 3.0}) == 3.0 && median_offset({4.0, 1.0, 2.0, 10.0}) == 3.0);
    const EssentialRanges live = essential_ranges(d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, d.ranges, d.sp);
    CHECK(live.index == d.live.index && !live.index.empty());
    CHECK(live.est_first == d.live.est_first && live.gyro_first == d.live.gyro_first);
    CHECK(live.est_has == d.live.est_has && live.gyro_has == d.live.gyro_has);
    CHECK(same(live.est, d.live.est) && same(live.gyro, d.live.gyro));
    std::printf("validate ok: %zu of %zu ranges reach the search\n", live.index.size(), d.ranges.size());
    return 0;
}

static int run_search(const Dump &d) {
    const int W = 64, H = 32;
    KernelParams cp;
    std::memset(&cp, 0, sizeof(cp));
    cp.width = cp.output_width = W; cp.height = cp.output_height = H; cp.stride = cp.output_stride = W;
    cp.f[0] = cp.f[1] = 0.47f * W; cp.c[0] = W / 2.0f; cp.c[1] = H / 2.0f;
    cp.input_vertical_stretch = 1.0f; cp.input_horizontal_stretch = 1.0f; cp.light_refraction_coefficient = 1.0f; cp.lens_correction_amount = 1.0f; cp.fov = 1.0f;
    cp.bytes_per_pixel = 1; cp.pix_element_count = 1; cp.interpolation = 2; cp.matrix_count = 1; cp.max_pixel_value = cp.pixel_value_limit = 255.0f;
    std::vector<uint8_t> src((size_t)W * H), dst((size_t)W * H);
    Buffers b;
    b.input.size = {W, H, W}; b.input.data = BufferSource::cpu(src.data(), src.size());
    b.output.size = {W, H, W}; b.output.data = BufferSource::cpu(dst.data(), dst.size());
    const gfw_buffers ab = b.to_abi();
    gfw_ctx *ctx = gfw_create(&cp, Luma8::ID, GFW_MODEL_OPENCV_FISHEYE, GFW_MODEL_NONE, &ab, 0);
    CHECK(ctx != nullptr);
    const auto found = find_offsets_essential(ctx, d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, d.ranges, d.sp);
    CHECK(std::string(gfw_last_backend(ctx)) == "sync_gyro_search");
    CHECK(found.size() == d.offsets.size() && !found.empty());
    for (size_t i = 0; i < found.size(); ++i) CHECK(found[i] == d.offsets[i]);
    const SyncParams fast = initial_offset_fast(ctx, d.estimated_gyro, d.raw_imu, d.duration_ms, d.fps, d.ranges, d.sp);
    CHECK(fast.initial_offset == d.fast.initial_offset && fast.search_size == 3000.0 && d.fast.search_size == 3000.0);
    std::printf("search ok: %zu offsets, first %.2f ms (cost %g); fast initial offset %.3f ms\n", found.size(), std::get<1>(found[0]), std::get<2>(found[0]), fast.initial_offset);
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::string(argv[1]) == "validate") return run_validate(load(argv[2]));
    if (argc >= 3 && std::string(argv[1]) == "search") return run_search(load(argv[2]));
    std::printf("usage: test_sync_gyro validate | search <dump>\n");
    return 2;
}
