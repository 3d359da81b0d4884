// C++ use of gyroflow::calculate_fovs (include/gfwarp.hpp): the adaptive-zoom fov series of a clip, the way recompute_adaptive_zoom asks for it.
//
//   test_zoom validate   error behaviour without a context, the empty clip; needs no GPU
//   test_zoom fovs       a 12-frame fisheye clip with caller-given rotations (identity and a small roll) on the device: static zoom = the minimum
//                        everywhere, a larger roll never gives a larger fov, disabled zoom = 1.0
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
    p.input_vertical_stretch = 1.0f; p.input_horizontal_stretch = 1.0f; p.light_refraction_coefficient = 1.0f;
    return p;
}
static std::vector<gfw_zoom_frame> clip(int n) {
    std::vector<gfw_zoom_frame> frames((size_t)n);
    for (int k = 0; k < n; ++k) {
        gfw_zoom_frame &f = frames[(size_t)k];
        std::memset(&f, 0, sizeof(f));
        f.timestamp_ms = 1000.0 + 33.3 * k;
        f.new_k[0] = f.new_k[4] = 0.47 * W; f.new_k[2] = W / 2.0; f.new_k[5] = H / 2.0; f.new_k[8] = 1.0;
        f.fov = 1.0; f.lens_correction_amount = 1.0;
    }
    return frames;
}

static int run_validate() {
    const KernelParams p = points_params();
    const gfw_zoom_search search = {W, H, W, H, 0.0f, 0};
    const auto empty = calculate_fovs(nullptr, p, search, {}, 1.0, 30.0, ZoomMethod::GaussianFilter);
    CHECK(empty.first.empty() && empty.second.empty());
    try { calculate_fovs(nullptr, p, search, clip(3), 1.0, 30.0, ZoomMethod::GaussianFilter); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(e.kind == GyroflowCoreError::Unknown && std::string(e.what()).find("zoom") != std::string::npos); }
    std::printf("validate ok\n");
    return 0;
}

static int run_fovs() {
    const int n = 12;
    KernelParams p = points_params();
    const gfw_zoom_search search = {W, H, W, H, 0.0f, 0};
    std::vector<uint8_t> src((size_t)W * H), dst((size_t)W * H);
    Buffers b;
    b.input.size = {W, H, W}; b.input.data = BufferSource::cpu(src.data(), src.size());
    b.output.size = {W, H, W}; b.output.data = BufferSource::cpu(dst.data(), dst.size());
    KernelParams cp = p;
    cp.stride = cp.output_stride = W; cp.bytes_per_pixel = 1; cp.pix_element_count = 1; cp.interpolation = 2; cp.matrix_count = 1;
    cp.max_pixel_value = cp.pixel_value_limit = 255.0f; cp.fov = 1.0f; cp.lens_correction_amount = 1.0f;
    const gfw_buffers ab = b.to_abi();
    gfw_ctx *ctx = gfw_create(&cp, Luma8::ID, GFW_MODEL_OPENCV_FISHEYE, GFW_MODEL_NONE, &ab, 0);
    CHECK(ctx != nullptr);
    const std::vector<gfw_zoom_frame> frames = clip(n);
    std::vector<float> rot((size_t)n * 9);
    for (int k = 0; k < n; ++k) {                                           // new_k * R: a roll about the optical axis growing with k (frame 0: identity)
        const double a = 0.01 * k, c = std::cos(a), s = std::sin(a), f = 0.47 * W;
        const double m[9] = {f * c, -f * s, W / 2.0, f * s, f * c, H / 2.0, 0.0, 0.0, 1.0};
        for (int i = 0; i < 9; ++i) rot[(size_t)k * 9 + i] = (float)m[i];
    }
    const auto fixed = calculate_fovs(ctx, p, search, frames, -1.0, 30.0, ZoomMethod::GaussianFilter, {}, rot.data());
    double mn = fixed.second[0];
    for (int k = 0; k < n; ++k) {
        CHECK(fixed.second[k] > 0.5 && fixed.second[k] < 2.0);
        if (k) CHECK(fixed.second[k] <= fixed.second[k - 1]);
        mn = std::fmin(mn, fixed.second[k]);
    }
    CHECK(fixed.second[n - 1] < fixed.second[0]);
    for (int k = 0; k < n; ++k) CHECK(fixed.first[k] == mn);
    const auto off = calculate_fovs(ctx, p, search, frames, 0.0, 30.0, ZoomMethod::GaussianFilter, {}, rot.data());
    const auto dyn = calculate_fovs(ctx, p, search, frames, 0.2, 30.0, ZoomMethod::EnvelopeFollower, {{0.0, 0.5}}, rot.data());
    for (int k = 0; k < n; ++k) { CHECK(off.first[k] == 1.0 && off.second[k] == fixed.second[k]); CHECK(dyn.first[k] <= dyn.second[k]); }
    CHECK(dyn.second[n - 1] == fixed.second[0]);                            // outside the trim range: the maximum
    CHECK(std::string(gfw_last_backend(ctx)) == "zoom_fovs");
    std::printf("fovs ok: minimal %.6f .. %.6f\n", fixed.second[n - 1], fixed.second[0]);
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "validate") return run_validate();
    if (argc >= 2 && std::string(argv[1]) == "fovs") return run_fovs();
    std::printf("usage: test_zoom validate | fovs\n");
    return 2;
}
