// C++ use of gyroflow::OptimSync (include/gfwarp.hpp): where in a clip to sync, against a dump of the numpy statements' results for a planted clip
// (tests/test_cpp_sync_optim.py writes it; numbers as C hex floats, so nothing is rounded on the way).
//
//   test_sync_optim validate <dump>   the host half: make() from raw samples equals the statement's resampling to the bit, nullopt without samples, the loud
//                                     failure without a context; needs no GPU
//   test_sync_optim run <dump>        run() on the device: points, rank and ratio equal the f32 statement's to the bit
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "gfwarp.hpp"

using namespace gyroflow;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

struct Dump {
    std::vector<TimeIMU> raw_imu;
    double sample_rate = 0.0, ratio = 0.0;
    std::array<std::vector<double>, 3> gyro;
    size_t target = 0;
    std::vector<std::pair<double, double>> trims;
    std::vector<double> points;
    std::vector<float> rank;
};
static double num(std::ifstream &f) { std::string s; CHECK(static_cast<bool>(f >> s)); return std::strtod(s.c_str(), nullptr); }
static long long integer(std::ifstream &f) { long long v = 0; CHECK(static_cast<bool>(f >> v)); return v; }
static Dump load(const char *path) {
    std::ifstream f(path);
    CHECK(f.good());
    Dump d;
    for (long long n = integer(f); n > 0; --n) { TimeIMU x; x.timestamp_ms = num(f); x.has_gyro = integer(f) != 0; for (int a = 0; a < 3; ++a) x.gyro[a] = num(f); d.raw_imu.push_back(x); }
    d.sample_rate = num(f);
    const long long s = integer(f);
    for (int a = 0; a < 3; ++a) for (long long i = 0; i < s; ++i) d.gyro[a].push_back(num(f));
    d.target = (size_t)integer(f);
    for (long long n = integer(f); n > 0; --n) { const double a = num(f), b = num(f); d.trims.emplace_back(a, b); }
    for (long long n = integer(f); n > 0; --n) d.points.push_back(num(f));
    for (long long n = integer(f); n > 0; --n) d.rank.push_back((float)num(f));
    d.ratio = num(f);
    return d;
}
template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static int run_validate(const Dump &d) {
    CHECK(!OptimSync::make({}).has_value());                                  // raw_imu.last()? (:34)
    const auto o = OptimSync::make(d.raw_imu);
    CHECK(o.has_value() && o->sample_rate == d.sample_rate);
    for (int a = 0; a < 3; ++a) CHECK(same(o->gyro[a], d.gyro[a]) && !o->gyro[a].empty());
    TimeIMU lone; lone.timestamp_ms = 5.0; lone.has_gyro = true;
    const auto single = OptimSync::make({lone});                              // one sample: no duration, no samples
    CHECK(single.has_value() && single->gyro[0].empty() && single->sample_rate > 1e300);
    try { o->run(nullptr, d.target, d.trims); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("sync") != std::string::npos); }
    std::printf("validate ok: %zu samples at %.3f Hz\n", o->gyro[0].size(), o->sample_rate);
    return 0;
}

static int run_device(const Dump &d) {
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
    const auto o = OptimSync::make(d.raw_imu);
    CHECK(o.has_value());
    const auto [points, rank, ratio] = o->run(ctx, d.target, d.trims);
    CHECK(std::string(gfw_last_backend(ctx)) == "sync_optim_points");
    CHECK(same(points, d.points) && !points.empty() && same(rank, d.rank) && ratio == d.ratio);
    const auto none = o->run(ctx, d.target, {});                              // `any` over nothing
    CHECK(std::get<0>(none).empty() && same(std::get<1>(none), d.rank));
    std::printf("run ok: %zu points, first %.1f ms; %zu windows\n", points.size(), points[0], rank.size());
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::string(argv[1]) == "validate") return run_validate(load(argv[2]));
    if (argc >= 3 && std::string(argv[1]) == "run") return run_device(load(argv[2]));
    std::printf("usage: test_sync_optim validate | run <dump>\n");
    return 2;
}
