// C++ use of the gyroflow::calculate_fovs overload for clips with stabiliser data and lens meshes (include/gfwarp.hpp, over gfw_zoom_fovs_stab).
//
//   test_zoom_stab validate   the empty clip, tables of the wrong length, the loud failure without a context; needs no GPU
//   test_zoom_stab fovs       a 12-frame fisheye clip with caller-given rotations on the device: empty tables give the plain overload's series, tables give
//                             gfw_zoom_fovs_stab's own, a frame without an entry keeps the plain value, a bad spline is reported with its frame
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
// a focal-plane-distortion block alone (mesh[0] = 9 <= 10: no grid), strength s
static std::vector<double> fpd_mesh(double s) {
    std::vector<double> m(40, 0.0);
    m[0] = 9.0; m[1] = 9.0; m[2] = 9.0; m[3] = W; m[4] = H; m[7] = W; m[8] = H;
    m[9] = 1.0;
    for (int i = 0; i < 8; ++i) { m[(size_t)(13 + i * 2)] = s * 0.002 * (i - 3); m[(size_t)(14 + i * 2)] = -s * 0.001 * (i - 4); }
    return m;
}

static int run_validate() {
    const KernelParams p = points_params();
    const gfw_zoom_search search = {W, H, W, H, 0.0f, 0};
    const std::vector<const gfw_frame_stab *> no_stabs;
    const std::vector<std::vector<double>> no_meshes;
    const auto empty = calculate_fovs(nullptr, p, search, {}, no_stabs, no_meshes, 1.0, 30.0, ZoomMethod::GaussianFilter);
    CHECK(empty.first.empty() && empty.second.empty());
    try { calculate_fovs(nullptr, p, search, clip(3), std::vector<const gfw_frame_stab *>(2, nullptr), no_meshes, 1.0, 30.0, ZoomMethod::GaussianFilter); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("per frame") != std::string::npos); }
    try { calculate_fovs(nullptr, p, search, clip(3), no_stabs, no_meshes, 1.0, 30.0, ZoomMethod::GaussianFilter); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("zoom") != std::string::npos); }
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
    for (int k = 0; k < n; ++k) {
        const double a = 0.01 * k, c = std::cos(a), s = std::sin(a), f = 0.47 * W;
        const double m[9] = {f * c, -f * s, W / 2.0, f * s, f * c, H / 2.0, 0.0, 0.0, 1.0};
        for (int i = 0; i < 9; ++i) rot[(size_t)k * 9 + i] = (float)m[i];
    }
    const auto plain = calculate_fovs(ctx, p, search, frames, -1.0, 30.0, ZoomMethod::GaussianFilter, {}, rot.data());
    const auto same = calculate_fovs(ctx, p, search, frames, {}, {}, -1.0, 30.0, ZoomMethod::GaussianFilter, {}, rot.data());
    CHECK(std::string(gfw_last_backend(ctx)) == "zoom_fovs");
    for (int k = 0; k < n; ++k) CHECK(same.first[k] == plain.first[k] && same.second[k] == plain.second[k]);
    // every frame but 5 distorts through one of two meshes; frames 0..5 name the first, 6..11 the second
    const std::vector<std::vector<double>> meshes = {fpd_mesh(40.0), fpd_mesh(-60.0)};
    std::vector<int> mesh_of_frame((size_t)n);
    for (int k = 0; k < n; ++k) mesh_of_frame[(size_t)k] = k == 5 ? -1 : k / 6;
    // ... and the even frames carry an IBIS spline (a constant shift of one pixel to the right and down)
    const double ibis[3 * 4] = {-1000.0, 54.0, 45.0, 0.0, 1500.0, 54.0, 45.0, 0.0, 9000.0, 54.0, 45.0, 0.0};
    gfw_frame_stab st;
    std::memset(&st, 0, sizeof(st));
    st.sensor_size[0] = 6000.0; st.sensor_size[1] = 3376.0;
    st.crop_area[0] = 120.0; st.crop_area[1] = 338.0; st.crop_area[2] = 5760.0; st.crop_area[3] = 2700.0;
    st.pixel_pitch[0] = st.pixel_pitch[1] = 3.0; st.width = W; st.height = H; st.ibis_count = 3; st.ibis = ibis;
    std::vector<const gfw_frame_stab *> stabs((size_t)n, nullptr);
    for (int k = 0; k < n; k += 2) stabs[(size_t)k] = &st;
    const auto got = calculate_fovs(ctx, p, search, frames, stabs, meshes, -1.0, 30.0, ZoomMethod::GaussianFilter, {}, rot.data(), mesh_of_frame);
    CHECK(std::string(gfw_last_backend(ctx)) == "zoom_fovs_stab");
    std::vector<const double *> mp((size_t)n); std::vector<size_t> ml((size_t)n);
    for (int k = 0; k < n; ++k) { const int m = mesh_of_frame[(size_t)k]; mp[(size_t)k] = m < 0 ? nullptr : meshes[(size_t)m].data(); ml[(size_t)k] = m < 0 ? 0 : meshes[(size_t)m].size(); }
    std::vector<double> direct((size_t)n);
    CHECK(gfw_zoom_fovs_stab(ctx, &p, &search, frames.data(), n, rot.data(), stabs.data(), mp.data(), ml.data(), direct.data(), nullptr, 0) == GFW_OK);
    int moved = 0;
    for (int k = 0; k < n; ++k) { CHECK(got.second[k] == direct[(size_t)k]); CHECK(got.second[k] > 0.5 && got.second[k] < 2.0); moved += got.second[k] != plain.second[k]; }
    CHECK(got.second[5] == plain.second[5]);                                // no mesh, no entry: the plain frame
    CHECK(moved >= 6);
    // a bad spline is reported with its frame
    const double down[3 * 4] = {100.0, 1.0, 1.0, 0.0, 50.0, 1.0, 1.0, 0.0, 200.0, 1.0, 1.0, 0.0};
    gfw_frame_stab bad = st;
    bad.ibis = down;
    stabs[4] = &bad;
    try { calculate_fovs(ctx, p, search, frames, stabs, meshes, -1.0, 30.0, ZoomMethod::GaussianFilter, {}, rot.data(), mesh_of_frame); CHECK(!"expected GyroflowCoreError"); }
    catch (const GyroflowCoreError &e) { CHECK(std::string(e.what()).find("frame 4") != std::string::npos); }
    std::printf("fovs ok: minimal %.6f .. %.6f\n", got.second[n - 1], got.second[0]);
    gfw_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "validate") return run_validate();
    if (argc >= 2 && std::string(argv[1]) == "fovs") return run_fovs();
    std::printf("usage: test_zoom_stab validate | fovs\n");
    return 2;
}
