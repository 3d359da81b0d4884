// C++ use of gyroflow::optical_flow_dis (include/gfwarp.hpp) with its trailing variational_iters: the DIS dense flow refined on every level (gfw_flow_dis_refined),
// against a dump of the numpy statement's results (tests/test_gpu_varref.py writes it in tests/test_cpp_dis.py's format: numbers as C hex floats, the frames as raw
// bytes in a file of their own; the wanted points are the REFINED statement's at the finest scales 2 and 1).
//
//   test_varref flow <dump> <frames>    every pair's points equal to the refined statement's to the bit at both finest scales; 0 iterations is gfw_flow_dis
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "gfwarp.hpp"

using namespace gyroflow;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

struct Dump {
    KernelParams kp;
    int model = 0, digital = 0, n_frames = 0, width = 0, height = 0, stride = 0;
    std::vector<std::pair<int, int>> pairs;
    std::vector<FlowPair> want2, want1;
    std::vector<uint8_t> frames;
};
static double num(std::ifstream &f) { std::string s; CHECK(static_cast<bool>(f >> s)); return std::strtod(s.c_str(), nullptr); }
static long long integer(std::ifstream &f) { long long v = 0; CHECK(static_cast<bool>(f >> v)); return v; }
static std::vector<FlowPair> wanted(std::ifstream &f, size_t n) {
    std::vector<FlowPair> out(n);
    for (auto &p : out) {
        p.has_points = integer(f) != 0;
        for (long long m = integer(f); m > 0; --m) { const float ax = (float)num(f), ay = (float)num(f), bx = (float)num(f), by = (float)num(f); p.points.emplace_back(ax, ay); p.next_points.emplace_back(bx, by); }
    }
    return out;
}
static Dump load(const char *path, const char *frames_path) {
    std::ifstream f(path);
    CHECK(f.good());
    Dump d;
    std::string hex;
    CHECK(static_cast<bool>(f >> hex) && hex.size() == 2 * sizeof(KernelParams));
    for (size_t i = 0; i < sizeof(KernelParams); ++i) ((unsigned char *)&d.kp)[i] = (unsigned char)std::strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    d.model = (int)integer(f); d.digital = (int)integer(f);
    d.n_frames = (int)integer(f); d.width = (int)integer(f); d.height = (int)integer(f); d.stride = (int)integer(f);
    for (long long n = integer(f); n > 0; --n) { const int a = (int)integer(f), b = (int)integer(f); d.pairs.emplace_back(a, b); }
    d.want2 = wanted(f, d.pairs.size());
    d.want1 = wanted(f, d.pairs.size());
    std::ifstream fr(frames_path, std::ios::binary);
    CHECK(fr.good());
    d.frames.resize((size_t)d.n_frames * d.height * d.stride);
    fr.read((char *)d.frames.data(), (std::streamsize)d.frames.size());
    CHECK((size_t)fr.gcount() == d.frames.size());
    return d;
}

// -> the number of points that differ in their destination
static size_t differing(const std::vector<FlowPair> &got, const std::vector<FlowPair> &want) {
    CHECK(got.size() == want.size());
    size_t with = 0, differ = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].has_points == want[i].has_points);
        if (!got[i].has_points) continue;
        ++with;
        CHECK(got[i].points.size() == want[i].points.size() && got[i].next_points.size() == want[i].next_points.size());
        for (size_t k = 0; k < got[i].points.size(); ++k) {
            CHECK(std::memcmp(&got[i].points[k], &want[i].points[k], sizeof(got[i].points[k])) == 0);
            differ += std::memcmp(&got[i].next_points[k], &want[i].next_points[k], sizeof(got[i].next_points[k])) != 0;
        }
    }
    CHECK(with > 0);
    return differ;
}

static int run_flow(const Dump &d) {
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
    CHECK(differing(optical_flow_dis(ctx, d.frames.data(), d.n_frames, d.width, d.height, d.stride, d.pairs, 2, 5), d.want2) == 0);
    CHECK(std::string(gfw_last_backend(ctx)) == "flow_dis_refined");
    CHECK(differing(optical_flow_dis(ctx, d.frames.data(), d.n_frames, d.width, d.height, d.stride, d.pairs, 1, 5), d.want1) == 0);
    // the default stays the unrefined gfw_flow_dis: other destinations
    CHECK(differing(optical_flow_dis(ctx, d.frames.data(), d.n_frames, d.width, d.height, d.stride, d.pairs), d.want2) > 0);
    CHECK(std::string(gfw_last_backend(ctx)) == "flow_dis");
    try { optical_flow_dis(ctx, d.frames.data(), d.n_frames, d.width, d.height, d.stride, d.pairs, 2, 65); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("fixed_point_iters 65") != std::string::npos); }
    std::printf("flow ok: %zu pairs\n", d.pairs.size());
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && std::string(argv[1]) == "flow") return run_flow(load(argv[2], argv[3]));
    std::printf("usage: test_varref flow <dump> <frames>\n");
    return 2;
}
