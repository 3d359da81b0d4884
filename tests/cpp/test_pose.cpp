// C++ use of gyroflow::estimate_poses_almeida / estimated_gyro (include/gfwarp.hpp): Almeida pose estimation of a clip's frame pairs and the series made of its
// rotations, against a dump of the numpy statement's results (tests/test_cpp_pose.py writes it; numbers as C hex floats, so nothing is rounded on the way).
//
//   test_pose validate <dump>   pairs without points need no context, pairs with points fail loudly without one; estimated_gyro — mid-point timestamps, the x / y
//                               swap in degrees, the final pass's interpolation, the low-pass — equal to the Python mirror's; scaled_axis; needs no GPU
//   test_pose estimate <dump>   estimate_poses_almeida on the device: quaternions and rotations equal to the statement's to the bit, euler to 1e-12
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "gfwarp.hpp"

using namespace gyroflow;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

struct Dump {
    KernelParams kp;
    int model = 0, digital = 0;
    gfw_pose_almeida_cfg cfg;
    double scaled_fps = 0.0, every_nth = 1.0;
    uint64_t seed = 0;
    std::vector<FlowPair> pairs;
    std::vector<PoseResult> want;
    std::map<int64_t, std::optional<std::array<double, 3>>> results;
    double fps = 0.0, lpf = 0.0;
    bool final_pass = false;
    std::map<int64_t, TimeIMU> gyro;
};
static double num(std::ifstream &f) { std::string s; CHECK(static_cast<bool>(f >> s)); return std::strtod(s.c_str(), nullptr); }
static long long integer(std::ifstream &f) { long long v = 0; CHECK(static_cast<bool>(f >> v)); return v; }
static Dump load(const char *path) {
    std::ifstream f(path);
    CHECK(f.good());
    Dump d;
    std::string hex;
    CHECK(static_cast<bool>(f >> hex) && hex.size() == 2 * sizeof(KernelParams));
    for (size_t i = 0; i < sizeof(KernelParams); ++i) ((unsigned char *)&d.kp)[i] = (unsigned char)std::strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    d.model = (int)integer(f); d.digital = (int)integer(f);
    std::memset(&d.cfg, 0, sizeof(d.cfg));
    d.cfg.video_width = (int32_t)integer(f); d.cfg.video_height = (int32_t)integer(f); d.cfg.flow_width = (int32_t)integer(f); d.cfg.flow_height = (int32_t)integer(f);
    d.cfg.num_iters = (int32_t)integer(f); d.cfg.num_samples = (int32_t)integer(f); d.cfg.inlier_angle_deg = (float)num(f);
    for (int i = 0; i < 9; ++i) d.cfg.camera_matrix[i] = num(f);
    d.scaled_fps = num(f); d.every_nth = num(f); d.seed = (uint64_t)integer(f);
    for (long long n = integer(f); n > 0; --n) {
        FlowPair p;
        p.has_points = integer(f) != 0;
        for (long long m = integer(f); m > 0; --m) { const float ax = (float)num(f), ay = (float)num(f), bx = (float)num(f), by = (float)num(f); p.points.emplace_back(ax, ay); p.next_points.emplace_back(bx, by); }
        d.pairs.push_back(p);
        PoseResult r;
        r.has_rotation = integer(f) != 0;
        for (int i = 0; i < 4; ++i) r.quat[i] = (float)num(f);
        for (int i = 0; i < 9; ++i) r.rotation[i] = num(f);
        for (int i = 0; i < 3; ++i) r.euler[i] = num(f);
        r.inliers = (int)integer(f); r.round = (int)integer(f);
        d.want.push_back(r);
    }
    for (long long n = integer(f); n > 0; --n) {
        const int64_t ts = integer(f);
        const bool has = integer(f) != 0;
        std::array<double, 3> e{num(f), num(f), num(f)};
        d.results[ts] = has ? std::optional<std::array<double, 3>>(e) : std::nullopt;
    }
    d.fps = num(f); d.lpf = num(f); d.final_pass = integer(f) != 0;
    for (long long n = integer(f); n > 0; --n) { const int64_t ts = integer(f); TimeIMU x; x.has_gyro = true; x.timestamp_ms = num(f); for (int a = 0; a < 3; ++a) x.gyro[a] = num(f); d.gyro[ts] = x; }
    return d;
}

static int run_validate(const Dump &d) {
    std::vector<FlowPair> none(3);
    const auto empty = estimate_poses_almeida(nullptr, d.kp, d.cfg, none, d.scaled_fps);
    CHECK(empty.size() == 3 && !empty[0].has_rotation && !empty[2].has_rotation);
    try { estimate_poses_almeida(nullptr, d.kp, d.cfg, d.pairs, d.scaled_fps); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("pose") != std::string::npos); }
    const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, quarter[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    CHECK(scaled_axis(ident) == (std::array<double, 3>{0.0, 0.0, 0.0}));
    const auto q = scaled_axis(quarter);
    CHECK(q[0] == 0.0 && q[1] == 0.0 && std::fabs(q[2] - 1.5707963267948966) < 1e-15);
    for (int pass = 0; pass < 2; ++pass) {
        const auto got = estimated_gyro(d.results, d.fps, pass ? d.lpf : 0.0, d.final_pass);
        CHECK(got.size() == d.gyro.size() && !got.empty());
        auto w = d.gyro.begin();
        for (auto g = got.begin(); g != got.end(); ++g, ++w) {
            CHECK(g->first == w->first && g->second.timestamp_ms == w->second.timestamp_ms && g->second.has_gyro);
            if (pass) for (int a = 0; a < 3; ++a) CHECK(g->second.gyro[a] == w->second.gyro[a]);
        }
    }
    std::printf("validate ok: %zu estimated samples of %zu frames\n", d.gyro.size(), d.results.size());
    return 0;
}

static int run_estimate(const Dump &d) {
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
    const auto got = estimate_poses_almeida(ctx, d.kp, d.cfg, d.pairs, d.scaled_fps, d.every_nth, d.seed);
    CHECK(std::string(gfw_last_backend(ctx)) == "pose_almeida");
    CHECK(got.size() == d.want.size());
    size_t rotated = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].has_rotation == d.want[i].has_rotation);
        if (!got[i].has_rotation) continue;
        CHECK(std::memcmp(got[i].quat, d.want[i].quat, sizeof(got[i].quat)) == 0);
        CHECK(std::memcmp(got[i].rotation, d.want[i].rotation, sizeof(got[i].rotation)) == 0);
        CHECK(got[i].inliers == d.want[i].inliers && got[i].round == d.want[i].round);
        for (int a = 0; a < 3; ++a) CHECK(std::fabs(got[i].euler[a] - d.want[i].euler[a]) <= 1e-12 * (1.0 + std::fabs(d.want[i].euler[a])));
        rotated += got[i].quat[0] != 1.0f;
    }
    CHECK(rotated > 0);
    std::printf("estimate ok: %zu pairs, %zu rotated\n", got.size(), rotated);
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::string(argv[1]) == "validate") return run_validate(load(argv[2]));
    if (argc >= 3 && std::string(argv[1]) == "estimate") return run_estimate(load(argv[2]));
    std::printf("usage: test_pose validate | estimate <dump>\n");
    return 2;
}
