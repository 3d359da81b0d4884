// C++ use of gyroflow::estimate_poses_essential (include/gfwarp.hpp): essential-matrix pose estimation of a clip's frame pairs, against a dump of the numpy
// statement's results (tests/test_cpp_pose_essential.py writes it; numbers as C hex floats, so nothing is rounded on the way).
//
//   test_pose_essential validate <dump>   pairs without points need no context, pairs with points fail loudly without one; needs no GPU
//   test_pose_essential estimate <dump>   estimate_poses_essential on the device: quaternions, rotations, essential matrices and best rounds equal to the
//                                         statement's to the bit, euler to 1e-12; a pair without a rotation has has_rotation = false
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
    gfw_pose_essential_cfg cfg;
    double scaled_fps = 0.0, every_nth = 1.0;
    uint64_t seed = 0;
    std::vector<FlowPair> pairs;
    std::vector<PoseEssentialResult> want;
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
    d.cfg.num_iters = (int32_t)integer(f); d.cfg.min_front = (int32_t)integer(f); d.cfg.inlier_threshold = num(f);
    for (int i = 0; i < 9; ++i) d.cfg.camera_matrix[i] = num(f);
    d.scaled_fps = num(f); d.every_nth = num(f); d.seed = (uint64_t)integer(f);
    for (long long n = integer(f); n > 0; --n) {
        FlowPair p;
        p.has_points = integer(f) != 0;
        for (long long m = integer(f); m > 0; --m) { const float ax = (float)num(f), ay = (float)num(f), bx = (float)num(f), by = (float)num(f); p.points.emplace_back(ax, ay); p.next_points.emplace_back(bx, by); }
        d.pairs.push_back(p);
        PoseEssentialResult r;
        r.has_rotation = integer(f) != 0;
        for (int i = 0; i < 4; ++i) r.quat[i] = (float)num(f);
        for (int i = 0; i < 9; ++i) r.rotation[i] = num(f);
        for (int i = 0; i < 9; ++i) r.essential[i] = num(f);
        for (int i = 0; i < 3; ++i) r.euler[i] = num(f);
        r.inliers = (int)integer(f); r.round = (int)integer(f); r.front = (int)integer(f);
        d.want.push_back(r);
    }
    return d;
}

static int run_validate(const Dump &d) {
    std::vector<FlowPair> none(3);
    const auto empty = estimate_poses_essential(nullptr, d.kp, d.cfg, none, d.scaled_fps);
    CHECK(empty.size() == 3 && !empty[0].has_rotation && !empty[2].has_rotation && empty[1].front == 0 && empty[1].rotation[0] == 1.0);
    try { estimate_poses_essential(nullptr, d.kp, d.cfg, d.pairs, d.scaled_fps); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("pose") != std::string::npos); }
    std::vector<FlowPair> odd(1);
    odd[0].has_points = true; odd[0].points.emplace_back(1.0f, 2.0f);
    try { estimate_poses_essential(nullptr, d.kp, d.cfg, odd, d.scaled_fps); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("one length") != std::string::npos); }
    std::printf("validate ok: %zu pairs\n", d.pairs.size());
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
    const auto got = estimate_poses_essential(ctx, d.kp, d.cfg, d.pairs, d.scaled_fps, d.every_nth, d.seed);
    CHECK(std::string(gfw_last_backend(ctx)) == "pose_essential");
    CHECK(got.size() == d.want.size());
    size_t rotated = 0, without = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].has_rotation == d.want[i].has_rotation);
        CHECK(std::memcmp(got[i].quat, d.want[i].quat, sizeof(got[i].quat)) == 0);
        CHECK(std::memcmp(got[i].rotation, d.want[i].rotation, sizeof(got[i].rotation)) == 0);
        CHECK(std::memcmp(got[i].essential, d.want[i].essential, sizeof(got[i].essential)) == 0);
        CHECK(got[i].inliers == d.want[i].inliers && got[i].round == d.want[i].round && got[i].front == d.want[i].front);
        for (int a = 0; a < 3; ++a) CHECK(std::fabs(got[i].euler[a] - d.want[i].euler[a]) <= 1e-12 * (1.0 + std::fabs(d.want[i].euler[a])));
        rotated += got[i].has_rotation && got[i].quat[0] != 1.0f;
        without += !got[i].has_rotation;
    }
    CHECK(rotated > 0 && without > 0);
    std::printf("estimate ok: %zu pairs, %zu rotated\n", got.size(), rotated);
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::string(argv[1]) == "validate") return run_validate(load(argv[2]));
    if (argc >= 3 && std::string(argv[1]) == "estimate") return run_estimate(load(argv[2]));
    std::printf("usage: test_pose_essential validate | estimate <dump>\n");
    return 2;
}
