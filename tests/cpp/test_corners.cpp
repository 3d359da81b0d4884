// C++ use of gyroflow::detect_features_pyrlk (include/gfwarp.hpp): Shi-Tomasi corner detection of a clip's frames, against a dump of the numpy statement's results
// (tests/test_cpp_corners.py writes it; numbers as C hex floats, so nothing is rounded on the way; the frames as raw bytes in a file of their own).
//
//   test_corners validate <dump> <frames>   no frames need no context, frames fail loudly without one; needs no GPU
//   test_corners detect <dump> <frames>     detect_features_pyrlk on the device: every frame's corners equal to the statement's to the bit, in pick order; then
//                                           optical_flow_pyrlk on them: every pair's kept points equal to the CPU chain's (the two statements) to the bit
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
    int model = 0, digital = 0, n_frames = 0, width = 0, height = 0, stride = 0;
    std::vector<std::vector<std::pair<float, float>>> corners;
    std::vector<std::pair<int, int>> pairs;
    std::vector<FlowPair> want;
    std::vector<uint8_t> frames;
};
static double num(std::ifstream &f) { std::string s; CHECK(static_cast<bool>(f >> s)); return std::strtod(s.c_str(), nullptr); }
static long long integer(std::ifstream &f) { long long v = 0; CHECK(static_cast<bool>(f >> v)); return v; }
static Dump load(const char *path, const char *frames_path) {
    std::ifstream f(path);
    CHECK(f.good());
    Dump d;
    std::string hex;
    CHECK(static_cast<bool>(f >> hex) && hex.size() == 2 * sizeof(KernelParams));
    for (size_t i = 0; i < sizeof(KernelParams); ++i) ((unsigned char *)&d.kp)[i] = (unsigned char)std::strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    d.model = (int)integer(f); d.digital = (int)integer(f);
    d.n_frames = (int)integer(f); d.width = (int)integer(f); d.height = (int)integer(f); d.stride = (int)integer(f);
    d.corners.resize((size_t)d.n_frames);
    for (auto &list : d.corners)
        for (long long m = integer(f); m > 0; --m) { const float x = (float)num(f), y = (float)num(f); list.emplace_back(x, y); }
    for (long long n = integer(f); n > 0; --n) { const int a = (int)integer(f), b = (int)integer(f); d.pairs.emplace_back(a, b); }
    d.want.resize(d.pairs.size());
    for (auto &p : d.want) {
        p.has_points = integer(f) != 0;
        for (long long m = integer(f); m > 0; --m) { const float ax = (float)num(f), ay = (float)num(f), bx = (float)num(f), by = (float)num(f); p.points.emplace_back(ax, ay); p.next_points.emplace_back(bx, by); }
    }
    std::ifstream fr(frames_path, std::ios::binary);
    CHECK(fr.good());
    d.frames.resize((size_t)d.n_frames * d.height * d.stride);
    fr.read((char *)d.frames.data(), (std::streamsize)d.frames.size());
    CHECK((size_t)fr.gcount() == d.frames.size());
    return d;
}

static int run_validate(const Dump &d) {
    CHECK(detect_features_pyrlk(nullptr, d.frames.data(), 0, d.width, d.height, d.stride).empty());
    try { detect_features_pyrlk(nullptr, d.frames.data(), d.n_frames, d.width, d.height, d.stride); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("corner detection") != std::string::npos); }
    std::printf("validate ok: %d frames\n", d.n_frames);
    return 0;
}

static int run_detect(const Dump &d) {
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
    const auto got = detect_features_pyrlk(ctx, d.frames.data(), d.n_frames, d.width, d.height, d.stride);
    CHECK(std::string(gfw_last_backend(ctx)) == "corners_shi_tomasi");
    CHECK(got.size() == d.corners.size());
    size_t total = 0;
    for (size_t f = 0; f < got.size(); ++f) {
        CHECK(got[f].size() == d.corners[f].size());
        for (size_t k = 0; k < got[f].size(); ++k) CHECK(std::memcmp(&got[f][k], &d.corners[f][k], sizeof(got[f][k])) == 0);
        total += got[f].size();
    }
    CHECK(total > 100);
    const auto flow = optical_flow_pyrlk(ctx, d.frames.data(), d.n_frames, d.width, d.height, d.stride, d.pairs, got);
    CHECK(flow.size() == d.want.size());
    for (size_t i = 0; i < flow.size(); ++i) {
        CHECK(flow[i].has_points && d.want[i].has_points && flow[i].points.size() == d.want[i].points.size());
        for (size_t k = 0; k < flow[i].points.size(); ++k) {
            CHECK(std::memcmp(&flow[i].points[k], &d.want[i].points[k], sizeof(flow[i].points[k])) == 0);
            CHECK(std::memcmp(&flow[i].next_points[k], &d.want[i].next_points[k], sizeof(flow[i].next_points[k])) == 0);
        }
    }
    try { detect_features_pyrlk(ctx, d.frames.data(), d.n_frames, 2, d.height, d.stride); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("frames of 2 x") != std::string::npos); }
    std::printf("detect ok: %zu corners of %d frames, %zu pairs\n", total, d.n_frames, flow.size());
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && std::string(argv[1]) == "validate") return run_validate(load(argv[2], argv[3]));
    if (argc >= 4 && std::string(argv[1]) == "detect") return run_detect(load(argv[2], argv[3]));
    std::printf("usage: test_corners validate | detect <dump> <frames>\n");
    return 2;
}
