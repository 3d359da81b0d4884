// gfwarp.hpp — C++ host-side mirror of gyroflow-core's operator surface for the warp path, on top of the C ABI
// (include/gfwarp.h).  Header-only, C++17, no HIP or torch types.
//
// The reference's host side is compiled Rust; its toolchain is not available here, so the host logic above the C ABI is
// restated in C++ with the reference's names, argument meaning and error behaviour:
//
//   gyroflow::Stabilization                src/core/stabilization/mod.rs:169-192
//     ::init_size                          mod.rs:375
//     ::get_kernel_flags                   mod.rs:226-251
//     ::get_frame_transform_at<T>          mod.rs:253-326   (completes KernelParams from the buffers and the pixel type)
//     ::ensure_ready_for_processing<T>     mod.rs:567-611   (backend object cache, LRU(15) as mod.rs:59-66)
//     ::process_pixels<T>                  mod.rs:612-725   (validation, then the backend arm; there is no CPU arm here)
//   gyroflow::BufferDescription / Buffers  src/core/gpu/mod.rs:17-28
//   gyroflow::FrameTransform               src/core/stabilization/frame_transform.rs:12-19
//   gyroflow::GyroflowCoreError            src/core/lib.rs:2099-2141
//   gyroflow::{Luma8, Luma16, ...}         src/core/stabilization/pixel_formats.rs (PixelType implementors)
//
//   gyroflow::calculate_fovs               src/core/zooming/mod.rs:35-70    (the adaptive-zoom fov series: one device call + host smoothing)
//   gyroflow::find_offsets_visual          src/core/synchronization/find_offset/visual_features.rs:10-147
//   gyroflow::find_offsets_essential       src/core/synchronization/find_offset/essential_matrix.rs:13-91   (+ initial_offset_fast: rs_sync.rs:26-45)
//   gyroflow::find_offsets_rssync          src/core/synchronization/find_offset/rs_sync.rs                  (the adapter; the rs-sync crate's solver is not reproduced)
//   gyroflow::OptimSync                    src/core/synchronization/optimsync.rs   (where in a clip to sync: new on the host, run in one device call)
//
// `FrameTransform::at_timestamp` itself (quaternions -> per-row matrices) is input here: the caller provides
// `matrices`, or builds them on the device with gfw_build_matrices / gfw_build_matrices_batch.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "gfwarp.h"

namespace gyroflow {

using KernelParams = gfw_kernel_params;
static_assert(sizeof(KernelParams) == 368, "KernelParams is #[repr(C, packed(4))], 368 bytes (mod.rs:101-150)");

enum class Interpolation : int32_t {                 // mod.rs:25-34
    Bilinear = 2, Bicubic = 4, Lanczos4 = 8, RobidouxSharp = 10, Robidoux = 11, Mitchell = 12, CatmullRom = 13
};

// GyroflowCoreError (lib.rs:2099-2141): the variants the pixel path can raise
struct GyroflowCoreError : std::runtime_error {
    enum Kind { SizeTooSmall, SizeMismatch, InvalidStride, NoStabilizationData, InputBufferEmpty, OutputBufferEmpty, Unknown };
    Kind kind;
    GyroflowCoreError(Kind k, const std::string &detail = "") : std::runtime_error(name(k) + (detail.empty() ? "" : ": " + detail)), kind(k) {}
    static std::string name(Kind k) {
        static const char *n[] = {"SizeTooSmall", "SizeMismatch", "InvalidStride", "NoStabilizationData", "InputBufferEmpty", "OutputBufferEmpty", "Unknown"};
        return n[k];
    }
    static Kind from_code(int rc) {
        switch (rc) {
        case GFW_ERR_SIZE_TOO_SMALL: return SizeTooSmall;
        case GFW_ERR_SIZE_MISMATCH: return SizeMismatch;
        case GFW_ERR_INVALID_STRIDE: return InvalidStride;
        case GFW_ERR_NO_STABILIZATION_DATA: return NoStabilizationData;
        case GFW_ERR_INPUT_BUFFER_EMPTY: return InputBufferEmpty;
        case GFW_ERR_OUTPUT_BUFFER_EMPTY: return OutputBufferEmpty;
        default: return Unknown;
        }
    }
};

// ---- PixelType implementors (pixel_formats.rs:48-60, :62-302): id, scalar type, element count, default_max_value ----
template <int Id, typename Scalar_, int Count_, bool HasMax, int MaxValue> struct PixelTypeT {
    static constexpr int ID = Id;
    using Scalar = Scalar_;
    static constexpr int COUNT = Count_;
    static constexpr int SCALAR_BYTES = (int)sizeof(Scalar_);
    static constexpr int BYTES = COUNT * SCALAR_BYTES;
    static std::optional<float> default_max_value() { return HasMax ? std::optional<float>((float)MaxValue) : std::nullopt; }
};
using Luma8   = PixelTypeT<GFW_PIX_LUMA8,   uint8_t,  1, true, 255>;
using Luma16  = PixelTypeT<GFW_PIX_LUMA16,  uint16_t, 1, true, 65535>;
using RGB8    = PixelTypeT<GFW_PIX_RGB8,    uint8_t,  3, true, 255>;
using RGBA8   = PixelTypeT<GFW_PIX_RGBA8,   uint8_t,  4, true, 255>;
using BGRA8   = PixelTypeT<GFW_PIX_BGRA8,   uint8_t,  4, true, 255>;
using RGB16   = PixelTypeT<GFW_PIX_RGB16,   uint16_t, 3, true, 65535>;
using RGBA16  = PixelTypeT<GFW_PIX_RGBA16,  uint16_t, 4, true, 65535>;
using AYUV16  = PixelTypeT<GFW_PIX_AYUV16,  uint16_t, 4, true, 65535>;
using RGBAf   = PixelTypeT<GFW_PIX_RGBAF,   float,    4, false, 0>;
using RGBAf16 = PixelTypeT<GFW_PIX_RGBAF16, uint16_t, 4, false, 0>;      // half::f16 storage
using R32f    = PixelTypeT<GFW_PIX_R32F,    float,    1, false, 0>;
using UV8     = PixelTypeT<GFW_PIX_UV8,     uint8_t,  2, true, 255>;
using UV16    = PixelTypeT<GFW_PIX_UV16,    uint16_t, 2, true, 65535>;

// ---- Buffers (gpu/mod.rs:17-71) ----
struct BufferSource {
    enum Kind { None, Cpu, HipDevice } kind = None;   // Cpu{buffer: &mut [u8]}; HipDevice = the CUDABuffer{buffer} analogue
    void *data = nullptr;
    size_t len = 0;
    static BufferSource cpu(void *p, size_t n) { return {Cpu, p, n}; }
    static BufferSource hip_device(void *p, size_t n) { return {HipDevice, p, n}; }
};
struct BufferDescription {
    std::tuple<size_t, size_t, size_t> size{0, 0, 0};                     // (width, height, stride in bytes)
    std::optional<std::tuple<size_t, size_t, size_t, size_t>> rect;       // (x, y, w, h)
    std::optional<float> rotation;
    BufferSource data;
    bool texture_copy = false;
    gfw_buffer_desc to_abi() const {
        gfw_buffer_desc d;
        std::memset(&d, 0, sizeof(d));
        d.width = (int32_t)std::get<0>(size); d.height = (int32_t)std::get<1>(size); d.stride = (int32_t)std::get<2>(size);
        if (rect) { d.has_rect = 1; d.rect[0] = (int32_t)std::get<0>(*rect); d.rect[1] = (int32_t)std::get<1>(*rect); d.rect[2] = (int32_t)std::get<2>(*rect); d.rect[3] = (int32_t)std::get<3>(*rect); }
        if (rotation) { d.has_rotation = 1; d.rotation = *rotation; }
        d.kind = data.kind == BufferSource::Cpu ? GFW_BUF_HOST : data.kind == BufferSource::HipDevice ? GFW_BUF_HIP_DEVICE : GFW_BUF_NONE;
        d.texture_copy = texture_copy ? 1 : 0;
        d.data = data.data; d.len = data.len;
        return d;
    }
};
struct Buffers {
    BufferDescription input, output;
    gfw_buffers to_abi() const { gfw_buffers b; b.input = input.to_abi(); b.output = output.to_abi(); return b; }
    // get_checksum (gpu/mod.rs:110-135): what makes a backend object reusable for another call
    uint64_t get_checksum() const {
        uint64_t h = 1469598103934665603ull;
        auto mix = [&h](uint64_t v) { h ^= v; h *= 1099511628211ull; };
        for (const BufferDescription *d : {&input, &output}) {
            mix(std::get<0>(d->size)); mix(std::get<1>(d->size)); mix(std::get<2>(d->size));
            mix(d->rect ? 1 : 0);
            if (d->rect) { mix(std::get<0>(*d->rect)); mix(std::get<1>(*d->rect)); mix(std::get<2>(*d->rect)); mix(std::get<3>(*d->rect)); }
            mix((uint64_t)d->data.kind);
        }
        return h;
    }
};

// ---- FrameTransform (frame_transform.rs:12-19) ----
struct FrameTransform {
    std::vector<std::array<float, 14>> matrices;
    KernelParams kernel_params{};
    double fov = 1.0, minimal_fov = 1.0;
    std::optional<double> focal_length;
    std::vector<float> mesh_data;
};
struct ProcessedInfo {                                                    // mod.rs:194-202
    double fov, minimal_fov;
    std::optional<double> focal_length;
    std::string backend;
};

// The slice of ComputeParams (compute_params.rs:71-138) that get_kernel_flags / the backend key consult
struct ComputeParams {
    int distortion_model = GFW_MODEL_OPENCV_FISHEYE;     // GFW_MODEL_* of params.distortion_model
    int digital_lens = GFW_MODEL_NONE;                   // params.digital_lens (None = GFW_MODEL_NONE)
    bool horizontal_rs = false;                          // frame_readout_direction.is_horizontal()
    bool framebuffer_inverted = false;
    float light_refraction_coefficient = 1.0f;
    std::array<float, 4> background{0.0f, 0.0f, 0.0f, 0.0f};
};

class Stabilization {
  public:
    std::pair<size_t, size_t> size{0, 0}, output_size{0, 0};
    Interpolation interpolation = Interpolation::Bilinear;
    int32_t kernel_flags = 0;
    ComputeParams compute_params;
    std::string initialized_backend;                                      // "" until a backend object exists

    ~Stabilization() { for (auto &e : backends_) gfw_destroy(e.second); }
    Stabilization() = default;
    Stabilization(const Stabilization &) = delete;
    Stabilization &operator=(const Stabilization &) = delete;

    void set_compute_params(const ComputeParams &p) { compute_params = p; }                        // mod.rs:204
    void init_size(std::pair<size_t, size_t> s, std::pair<size_t, size_t> out) { initialized_backend.clear(); size = s; output_size = out; }   // mod.rs:375

    static std::tuple<size_t, size_t, size_t, size_t> get_rect(const BufferDescription &d) {       // mod.rs:209-224
        if (d.rect) return *d.rect;
        return {0, 0, std::get<0>(d.size), std::get<1>(d.size)};
    }
    int32_t get_kernel_flags(const Buffers &b) const {                                             // mod.rs:226-251
        int32_t f = kernel_flags;
        auto set = [&f](int32_t bit, bool on) { f = on ? (f | bit) : (f & ~bit); };
        set(GFW_FLAG_HAS_DIGITAL_LENS, compute_params.digital_lens != GFW_MODEL_NONE);
        set(GFW_FLAG_HORIZONTAL_RS, compute_params.horizontal_rs);
        set(GFW_FLAG_HAS_SOURCE_RECT, b.input.rect.has_value() || size != std::make_pair(std::get<0>(b.input.size), std::get<1>(b.input.size)));
        set(GFW_FLAG_HAS_OUTPUT_RECT, b.output.rect.has_value() || output_size != std::make_pair(std::get<0>(b.output.size), std::get<1>(b.output.size)));
        set(GFW_FLAG_FRAMEBUFFER_INVERTED, compute_params.framebuffer_inverted);
        set(GFW_FLAG_ANY_UNDERWATER, compute_params.light_refraction_coefficient != 1.0f && compute_params.light_refraction_coefficient > 0.0f);
        return f;
    }

    // mod.rs:253-326: complete the per-frame KernelParams (lens, fov, matrix_count, ... already filled by
    // FrameTransform::at_timestamp, frame_transform.rs:322-340) from the buffers and the pixel type.
    template <typename T>
    FrameTransform get_frame_transform_at(FrameTransform transform, const Buffers &b) const {
        KernelParams &p = transform.kernel_params;
        p.pixel_value_limit = T::default_max_value().value_or(std::numeric_limits<float>::max());
        p.max_pixel_value = T::default_max_value().value_or(1.0f);
        p.interpolation = (int32_t)interpolation;                                                  // before the EWA test below
        p.width = (int32_t)size.first; p.height = (int32_t)size.second;
        p.output_width = (int32_t)output_size.first; p.output_height = (int32_t)output_size.second;
        for (int i = 0; i < 4; ++i) p.background[i] = compute_params.background[i];
        p.bytes_per_pixel = T::BYTES;
        p.pix_element_count = T::COUNT;
        p.canvas_scale = 1.0f;
        p.flags = get_kernel_flags(b);
        p.stride = (int32_t)std::get<2>(b.input.size);
        p.output_stride = (int32_t)std::get<2>(b.output.size);
        if (p.interpolation > 8) {                                                                 // mod.rs:279-295 (Keys cubic family)
            float B = 0.0f, C = 0.5f;
            switch (interpolation) {
            case Interpolation::RobidouxSharp: B = 0.2620145f; C = 0.3689927f; break;
            case Interpolation::Robidoux:      B = 0.3782157f; C = 0.3108921f; break;
            case Interpolation::Mitchell:      B = 0.3333333f; C = 0.3333333f; break;
            default:                           B = 0.0f;       C = 0.5f;       break;              // CatmullRom
            }
            p.ewa_coeffs_p[0] = (6.0f - 2.0f * B) / 6.0f;
            p.ewa_coeffs_p[1] = 0.0f;
            p.ewa_coeffs_p[2] = (-18.0f + 12.0f * B + 6.0f * C) / 6.0f;
            p.ewa_coeffs_p[3] = (12.0f - 9.0f * B - 6.0f * C) / 6.0f;
            p.ewa_coeffs_q[0] = (8.0f * B + 24.0f * C) / 6.0f;
            p.ewa_coeffs_q[1] = (-12.0f * B - 48.0f * C) / 6.0f;
            p.ewa_coeffs_q[2] = (6.0f * B + 30.0f * C) / 6.0f;
            p.ewa_coeffs_q[3] = (-1.0f * B - 6.0f * C) / 6.0f;
        }
        p.safe_area_rect[0] = 0.0f; p.safe_area_rect[1] = 0.0f;
        p.safe_area_rect[2] = (float)output_size.first; p.safe_area_rect[3] = (float)output_size.second;
        if (b.input.rotation) p.input_rotation = *b.input.rotation;
        if (b.output.rotation) p.output_rotation = *b.output.rotation;
        const auto sr = get_rect(b.input), orr = get_rect(b.output);
        p.source_rect[0] = (int32_t)std::get<0>(sr); p.source_rect[1] = (int32_t)std::get<1>(sr); p.source_rect[2] = (int32_t)std::get<2>(sr); p.source_rect[3] = (int32_t)std::get<3>(sr);
        p.output_rect[0] = (int32_t)std::get<0>(orr); p.output_rect[1] = (int32_t)std::get<1>(orr); p.output_rect[2] = (int32_t)std::get<2>(orr); p.output_rect[3] = (int32_t)std::get<3>(orr);
        return transform;
    }

    // mod.rs:355-373: what a backend object is keyed by (FILL_WITH_BACKGROUND stays a run-time flag, opencl.rs:209)
    uint64_t get_current_checksum(const Buffers &b, int pixel_type) const {
        uint64_t h = b.get_checksum();
        auto mix = [&h](uint64_t v) { h ^= v; h *= 1099511628211ull; };
        mix((uint64_t)compute_params.distortion_model); mix((uint64_t)compute_params.digital_lens);
        mix((uint64_t)(int32_t)interpolation);
        mix((uint64_t)(get_kernel_flags(b) & ~GFW_FLAG_FILL_WITH_BACKGROUND));
        mix(size.first); mix(size.second); mix(output_size.first); mix(output_size.second);
        mix((uint64_t)pixel_type);
        return h;
    }

    // mod.rs:567-611 (init_backends :467-565 restricted to the HIP arm): create or reuse the backend object
    template <typename T>
    gfw_ctx *ensure_ready_for_processing(const KernelParams &kp, const Buffers &b) {
        const uint64_t key = get_current_checksum(b, T::ID);
        for (auto it = backends_.begin(); it != backends_.end(); ++it)
            if (it->first == key) { backends_.splice(backends_.begin(), backends_, it); return backends_.front().second; }
        const gfw_buffers ab = b.to_abi();
        gfw_ctx *ctx = gfw_create(&kp, T::ID, compute_params.distortion_model, compute_params.digital_lens, &ab, 0);
        if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, std::string("backend initialisation failed: ") + gfw_last_error());
        backends_.emplace_front(key, ctx);
        while (backends_.size() > 15) { gfw_destroy(backends_.back().second); backends_.pop_back(); }   // LRU(15), mod.rs:59-66
        char info[256] = {0};
        initialized_backend = gfw_get_info(info, sizeof(info)) >= 0 ? std::string("HIP: ") + info : "HIP";
        return ctx;
    }

    // mod.rs:612-725.  `frame_transform` = None -> NoStabilizationData (this mirror keeps no stab_data cache).
    template <typename T>
    ProcessedInfo process_pixels(int64_t timestamp_us, std::optional<size_t> /*frame*/, Buffers &buffers, const FrameTransform *frame_transform) {
        if (std::get<1>(buffers.input.size) < 4 || std::get<1>(buffers.output.size) < 4) throw GyroflowCoreError(GyroflowCoreError::SizeTooSmall);   // :613
        if (!frame_transform) throw GyroflowCoreError(GyroflowCoreError::NoStabilizationData, std::to_string(timestamp_us));                       // :721
        const FrameTransform &itm = *frame_transform;
        const KernelParams &kp = itm.kernel_params;
        if (size != std::make_pair((size_t)kp.width, (size_t)kp.height)) throw GyroflowCoreError(GyroflowCoreError::SizeMismatch);                  // :636
        if (output_size != std::make_pair((size_t)kp.output_width, (size_t)kp.output_height)) throw GyroflowCoreError(GyroflowCoreError::SizeMismatch);
        if ((int64_t)std::get<0>(buffers.input.size) > kp.stride) throw GyroflowCoreError(GyroflowCoreError::InvalidStride);                         // :639
        if ((int64_t)std::get<0>(buffers.output.size) > kp.output_stride) throw GyroflowCoreError(GyroflowCoreError::InvalidStride);
        if (buffers.input.data.kind == BufferSource::None || buffers.input.data.len == 0) throw GyroflowCoreError(GyroflowCoreError::InputBufferEmpty);     // lib.rs:890
        if (buffers.output.data.kind == BufferSource::None || buffers.output.data.len == 0) throw GyroflowCoreError(GyroflowCoreError::OutputBufferEmpty);  // lib.rs:891
        gfw_ctx *ctx = ensure_ready_for_processing<T>(kp, buffers);
        const gfw_buffers ab = buffers.to_abi();
        const int rc = gfw_undistort_image(ctx, &ab, &kp, itm.matrices.empty() ? nullptr : itm.matrices[0].data(), (int)itm.matrices.size(), nullptr, 0,
                                           itm.mesh_data.empty() ? nullptr : itm.mesh_data.data(), itm.mesh_data.size());
        if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
        return ProcessedInfo{itm.fov, itm.minimal_fov, itm.focal_length, std::string("HIP:") + gfw_last_backend(ctx)};
    }

  private:
    std::list<std::pair<uint64_t, gfw_ctx *>> backends_;
};

// ---- zooming/mod.rs:35-70 `calculate_fovs` over the two C calls: gfw_zoom_fovs (FovIterative::find_fov of every frame, one device call) and gfw_zoom_smooth
// (static / dynamic / disabled zoom on the host).  `ctx`: a context of the clip's lens models whose tracks are set (gfw_set_quaternion_tracks), or
// `rotations` = one `new_k * R` (9 f32) per frame.  `params`, `search`, `frames`: see include/gfwarp.h.  -> (fovs, minimal fovs).
enum class ZoomMethod : int32_t { GaussianFilter = 0, EnvelopeFollower = 1 };                       // mod.rs:16-29
inline std::pair<std::vector<double>, std::vector<double>> calculate_fovs(gfw_ctx *ctx, const KernelParams &params, const gfw_zoom_search &search,
                                                                          const std::vector<gfw_zoom_frame> &frames, double adaptive_zoom_window, double scaled_fps,
                                                                          ZoomMethod method, const std::vector<std::pair<double, double>> &trim_ranges = {},
                                                                          const float *rotations = nullptr) {
    const int n = (int)frames.size();
    std::vector<double> minimal((size_t)n), fovs((size_t)n), trimmed((size_t)n), ranges;
    if (n == 0) return {fovs, minimal};                                                             // mod.rs:36-38
    int rc = gfw_zoom_fovs(ctx, &params, &search, frames.data(), n, rotations, minimal.data(), nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (const auto &r : trim_ranges) { ranges.push_back(r.first); ranges.push_back(r.second); }
    rc = gfw_zoom_smooth(minimal.data(), n, adaptive_zoom_window, scaled_fps, (int)method, ranges.empty() ? nullptr : ranges.data(), (int)trim_ranges.size(),
                         fovs.data(), trimmed.data());
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    return {fovs, trimmed};
}
// The same for a clip with stabiliser data and lens meshes, over gfw_zoom_fovs_stab: `stabs` = file_metadata.camera_stab_data, one pointer per frame (nullptr = no
// entry) or empty; `meshes` = mesh_correction[frame].0, the distorting mesh, one vector per frame (empty = none) or empty.  Consecutive frames whose meshes are equal
// share one upload when they are given as the same vector object through `mesh_of_frame` (index into `meshes` per frame; empty = frame f names meshes[f]).
inline std::pair<std::vector<double>, std::vector<double>> calculate_fovs(gfw_ctx *ctx, const KernelParams &params, const gfw_zoom_search &search,
                                                                          const std::vector<gfw_zoom_frame> &frames, const std::vector<const gfw_frame_stab *> &stabs,
                                                                          const std::vector<std::vector<double>> &meshes, double adaptive_zoom_window, double scaled_fps,
                                                                          ZoomMethod method, const std::vector<std::pair<double, double>> &trim_ranges = {},
                                                                          const float *rotations = nullptr, const std::vector<int> &mesh_of_frame = {}) {
    const int n = (int)frames.size();
    std::vector<double> minimal((size_t)n), fovs((size_t)n), trimmed((size_t)n), ranges;
    if (n == 0) return {fovs, minimal};
    if ((!stabs.empty() && (int)stabs.size() != n) || (!mesh_of_frame.empty() && (int)mesh_of_frame.size() != n) || (mesh_of_frame.empty() && !meshes.empty() && (int)meshes.size() != n))
        throw GyroflowCoreError(GyroflowCoreError::from_code(GFW_ERR_INVALID_ARGUMENT), "calculate_fovs: one stabiliser entry and one mesh per frame");
    std::vector<const double *> mesh_ptrs;
    std::vector<size_t> mesh_lens;
    if (!meshes.empty()) {
        mesh_ptrs.resize((size_t)n); mesh_lens.resize((size_t)n);
        for (int f = 0; f < n; ++f) {
            const int m = mesh_of_frame.empty() ? f : mesh_of_frame[(size_t)f];
            if (m >= (int)meshes.size()) throw GyroflowCoreError(GyroflowCoreError::from_code(GFW_ERR_INVALID_ARGUMENT), "calculate_fovs: mesh_of_frame names no mesh");
            mesh_ptrs[(size_t)f] = (m < 0 || meshes[(size_t)m].empty()) ? nullptr : meshes[(size_t)m].data();
            mesh_lens[(size_t)f] = m < 0 ? 0 : meshes[(size_t)m].size();
        }
    }
    int rc = gfw_zoom_fovs_stab(ctx, &params, &search, frames.data(), n, rotations, stabs.empty() ? nullptr : stabs.data(),
                                mesh_ptrs.empty() ? nullptr : mesh_ptrs.data(), mesh_lens.empty() ? nullptr : mesh_lens.data(), minimal.data(), nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (const auto &r : trim_ranges) { ranges.push_back(r.first); ranges.push_back(r.second); }
    rc = gfw_zoom_smooth(minimal.data(), n, adaptive_zoom_window, scaled_fps, (int)method, ranges.empty() ? nullptr : ranges.data(), (int)trim_ranges.size(),
                         fovs.data(), trimmed.data());
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    return {fovs, trimmed};
}

// ---- synchronization/find_offset/visual_features.rs:10-147 `find_offsets` over gfw_sync_visual_search: the offset (or, with for_rs, the frame readout time) of
// every range, one device call per range.  `ctx`: a context of the clip's lens models whose tracks are set (gfw_set_quaternion_tracks; with for_rs the sync offsets
// too: the offset search clears them, :13-15 — `search.use_sync_offsets` is set from for_rs here).  `matched`: what get_of_lines_for_timestamp returns for the keys of
// the estimator's sync results, ascending by timestamp; entries whose point sets are empty or of different lengths are skipped (:36-40).
// -> (timestamp, offset, cost) per range that has candidates and, for the offset search, passes the 90 %-of-range rule (:137).
struct SyncParams { double initial_offset = 0.0, search_size = 0.0; };                              // ms (synchronization/mod.rs)
struct MatchedPoints { int64_t timestamp_us = 0, next_timestamp_us = 0; std::vector<std::pair<float, float>> points, next_points; };
inline std::vector<std::tuple<double, double, double>> find_offsets_visual(gfw_ctx *ctx, const KernelParams &params, gfw_sync_search search,
                                                                           const std::vector<std::pair<int64_t, int64_t>> &ranges, const std::vector<MatchedPoints> &matched,
                                                                           const SyncParams &sync_params, double frame_readout_time_ms, double scaled_fps, bool for_rs = false) {
    std::vector<std::tuple<double, double, double>> final_offsets;
    search.use_sync_offsets = for_rs ? 1 : 0;
    for (const auto &range : ranges) {
        std::vector<int64_t> ts;
        std::vector<int32_t> first{0};
        std::vector<float> a, b;
        for (const MatchedPoints &m : matched) {
            if (m.timestamp_us < range.first || m.timestamp_us >= range.second) continue;             // (*from_ts..*to_ts).contains(ts)
            if (m.points.empty() || m.points.size() != m.next_points.size()) continue;
            ts.push_back(m.timestamp_us); ts.push_back(m.next_timestamp_us);
            for (const auto &pt : m.points) { a.push_back(pt.first); a.push_back(pt.second); }
            for (const auto &pt : m.next_points) { b.push_back(pt.first); b.push_back(pt.second); }
            first.push_back((int32_t)(a.size() / 2));
        }
        gfw_sync_result r;
        std::memset(&r, 0, sizeof(r));
        const int rc = gfw_sync_visual_search(ctx, &params, &search, ts.data(), first.data(), a.data(), b.data(), (int)(ts.size() / 2), for_rs ? 1 : 0,
                                              sync_params.initial_offset, sync_params.search_size, frame_readout_time_ms, scaled_fps, &r, nullptr, nullptr, 0);
        if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
        if (!r.found) continue;
        if (for_rs) { final_offsets.emplace_back(0.0, r.value, r.cost); continue; }                 // :109
        const double middle_timestamp = ((double)range.first + (double)(range.second - range.first) / 2.0) / 1000.0;
        const double d = r.value - sync_params.initial_offset;
        if ((d < 0.0 ? -d : d) < sync_params.search_size * 0.9) final_offsets.emplace_back(middle_timestamp, r.value, r.cost);       // :137
    }
    return final_offsets;
}

// ---- synchronization/find_offset/essential_matrix.rs:13-91 `find_offsets` over gfw_sync_gyro_search: the gyro-match offset of every range (offset method 0), ALL
// ranges in one device call; and rs_sync.rs:26-45, the fast initial offset rs-sync starts from.  `estimated_gyro`: the estimator's BTreeMap<i64 timestamp_us, TimeIMU>
// (the angular rates pose estimation produced — the caller's input); `raw_imu`: gyro.raw_imu(); `duration_ms`: gyro.duration_ms.  The guards (:22, :26), the range cut
// (`from_ts..to_ts`, the end excluded), the gyro window (:31-38), the max-angle skip (:40-44, on the unfiltered samples), the two 20 Hz low-pass calls
// (gfw_lowpass_gyro; a refusal — 2 * 20 > rate — is ignored as the reference ignores it), the 90 % rule (:81) and the middle timestamp (:78) are applied here.
struct TimeIMU { double timestamp_ms = 0.0; bool has_gyro = false; double gyro[3] = {0.0, 0.0, 0.0}; };
struct EssentialRanges {                                                                            // what gfw_sync_gyro_search takes, and which range each entry is
    std::vector<size_t> index;
    std::vector<int32_t> est_first{0}, gyro_first{0};
    std::vector<double> est, gyro;                                                                  // [][4] (timestamp_ms, x, y, z)
    std::vector<uint8_t> est_has, gyro_has;
};
namespace detail {
inline void essential_append(const std::vector<const TimeIMU *> &items, double rate, std::vector<int32_t> &first, std::vector<double> &rows, std::vector<uint8_t> &has) {
    std::vector<double> xyz(items.size() * 3);
    std::vector<uint8_t> h(items.size());
    for (size_t i = 0; i < items.size(); ++i) { h[i] = items[i]->has_gyro ? 1 : 0; for (int a = 0; a < 3; ++a) xyz[i * 3 + a] = items[i]->has_gyro ? items[i]->gyro[a] : 0.0; }
    const int rc = gfw_lowpass_gyro(20.0, rate, xyz.data(), h.data(), (int)items.size());           // `let _ =`: GFW_FILTER_NOT_APPLIED goes on unfiltered
    if (rc < 0) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (size_t i = 0; i < items.size(); ++i) {
        rows.push_back(items[i]->timestamp_ms); rows.push_back(xyz[i * 3]); rows.push_back(xyz[i * 3 + 1]); rows.push_back(xyz[i * 3 + 2]);
        has.push_back(h[i]);
    }
    first.push_back((int32_t)(rows.size() / 4));
}
}  // namespace detail
inline EssentialRanges essential_ranges(const std::map<int64_t, TimeIMU> &estimated_gyro, const std::vector<TimeIMU> &raw_imu, double duration_ms, double scaled_fps,
                                        const std::vector<std::pair<int64_t, int64_t>> &ranges, const SyncParams &sync_params) {
    EssentialRanges out;
    if (estimated_gyro.empty() || !(duration_ms > 0.0) || raw_imu.empty()) return out;              // :22
    for (size_t r = 0; r < ranges.size(); ++r) {
        if (ranges[r].second <= ranges[r].first) continue;                                          // :26
        std::vector<const TimeIMU *> of_item, gyro_item;
        for (auto it = estimated_gyro.lower_bound(ranges[r].first); it != estimated_gyro.end() && it->first < ranges[r].second; ++it) of_item.push_back(&it->second);
        if (of_item.empty()) continue;
        const double lo = of_item.front()->timestamp_ms - sync_params.search_size, hi = of_item.back()->timestamp_ms + sync_params.search_size;
        for (const TimeIMU &x : raw_imu) { const double ts = x.timestamp_ms + sync_params.initial_offset; if (ts >= lo && ts <= hi) gyro_item.push_back(&x); }
        double max_angle = 0.0;                                                                     // get_max_angle (:93-103)
        for (const TimeIMU *x : of_item) if (x->has_gyro) for (int a = 0; a < 3; ++a) { const double v = x->gyro[a] < 0.0 ? -x->gyro[a] : x->gyro[a]; if (v > max_angle) max_angle = v; }
        if (max_angle < 3.0) continue;
        const double sample_rate = (double)raw_imu.size() / (duration_ms / 1000.0);
        detail::essential_append(of_item, scaled_fps, out.est_first, out.est, out.est_has);
        detail::essential_append(gyro_item, sample_rate, out.gyro_first, out.gyro, out.gyro_has);
        out.index.push_back(r);
    }
    return out;
}
inline std::vector<std::tuple<double, double, double>> find_offsets_essential(gfw_ctx *ctx, const std::map<int64_t, TimeIMU> &estimated_gyro, const std::vector<TimeIMU> &raw_imu,
                                                                              double duration_ms, double scaled_fps, const std::vector<std::pair<int64_t, int64_t>> &ranges,
                                                                              const SyncParams &sync_params) {
    std::vector<std::tuple<double, double, double>> offsets;
    const EssentialRanges live = essential_ranges(estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params);
    if (live.index.empty()) return offsets;
    std::vector<gfw_sync_result> results(live.index.size());
    std::memset(results.data(), 0, sizeof(gfw_sync_result) * results.size());
    const int rc = gfw_sync_gyro_search(ctx, live.est_first.data(), live.est.data(), live.est_has.data(), (int)live.est_has.size(), live.gyro_first.data(), live.gyro.data(),
                                        live.gyro_has.data(), (int)live.gyro_has.size(), (int)live.index.size(), sync_params.initial_offset, sync_params.search_size,
                                        results.data(), nullptr, nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (size_t k = 0; k < live.index.size(); ++k) {
        if (!results[k].found) continue;
        const auto &range = ranges[live.index[k]];
        const double middle_timestamp = ((double)range.first + (double)(range.second - range.first) / 2.0) / 1000.0;      // :78
        const double d = results[k].value - sync_params.initial_offset;
        if ((d < 0.0 ? -d : d) < sync_params.search_size * 0.9) offsets.emplace_back(middle_timestamp, results[k].value, results[k].cost);       // :81
    }
    return offsets;
}
inline double median_offset(std::vector<double> v) {                                                // rs_sync.rs:27-35
    std::stable_sort(v.begin(), v.end(), [](double a, double b) { return a < b; });
    const size_t len = v.size();
    return len % 2 == 0 ? (v[len / 2 - 1] + v[len / 2]) / 2.0 : v[len / 2];
}
// -> the (initial_offset, search_size) rs-sync starts from: the median of the gyro-match offsets and 3000 ms, or the inputs unchanged when nothing was found
inline SyncParams initial_offset_fast(gfw_ctx *ctx, const std::map<int64_t, TimeIMU> &estimated_gyro, const std::vector<TimeIMU> &raw_imu, double duration_ms, double scaled_fps,
                                      const std::vector<std::pair<int64_t, int64_t>> &ranges, SyncParams sync_params) {
    if (ranges.empty() || raw_imu.empty()) return sync_params;
    const auto offsets = find_offsets_essential(ctx, estimated_gyro, raw_imu, duration_ms, scaled_fps, ranges, sync_params);
    if (offsets.empty()) return sync_params;
    std::vector<double> v;
    for (const auto &o : offsets) v.push_back(std::get<1>(o));
    sync_params.initial_offset = median_offset(v);
    sync_params.search_size = 3000.0;
    return sync_params;
}

// ---- synchronization/find_offset/rs_sync.rs `find_offsets` over gfw_sync_rs_search: the rs-sync offset of every range (offset method 2, the reference's default), ALL
// ranges in one device call.  The adapter is mirrored here — collect_points' range cut (:224-241), ranges under 2 pairs skipped (:108), the sign and unit
// conventions (:164-166, :176-179), the 90 %-of-radius rule (:178) and the middle timestamp (:180); the solver, the rs-sync crate, is not in the reference tree and is
// NOT reproduced (include/gfwarp.h says what runs instead).  `cfg.frame_readout_time_ms`: rs_readout_time_ms of the clip's; `matched` as for find_offsets_visual,
// ascending by timestamp; `track_*`: the gyro's quaternions (:159), timestamps strictly ascending, (w, x, y, z).  With calc_initial_fast the caller passes what
// initial_offset_fast returns as `sync_params`.  -> (timestamp, offset, cost) per range that is searched and accepted.
inline double rs_readout_time_ms(double frame_readout_time_ms, double scaled_fps, bool global_shutter) {      // :74-80
    double t = frame_readout_time_ms;
    if (t == 0.0) t = 1000.0 / scaled_fps / 2.0;
    if (global_shutter) t = 0.01;
    return t;
}
inline std::vector<std::tuple<double, double, double>> find_offsets_rssync(gfw_ctx *ctx, const KernelParams &params, const gfw_sync_rs_cfg &cfg,
                                                                           const std::vector<std::pair<int64_t, int64_t>> &ranges, const std::vector<MatchedPoints> &matched,
                                                                           const SyncParams &sync_params, const std::vector<int64_t> &track_timestamps_us,
                                                                           const std::vector<double> &track_wxyz) {
    std::vector<std::tuple<double, double, double>> offsets;
    if (track_wxyz.size() != track_timestamps_us.size() * 4) throw GyroflowCoreError(GyroflowCoreError::Unknown, "find_offsets_rssync: one (w, x, y, z) per track timestamp");
    std::vector<std::pair<int64_t, int64_t>> sync_points;
    std::vector<int32_t> range_first{0}, first{0};
    std::vector<int64_t> ts;
    std::vector<float> a, b;
    for (const auto &range : ranges) {
        std::vector<const MatchedPoints *> in;
        if (range.second > range.first)
            for (const MatchedPoints &m : matched) if (m.timestamp_us >= range.first && m.timestamp_us < range.second) in.push_back(&m);
        if (in.size() < 2) continue;                                                                // :108
        for (const MatchedPoints *m : in) {
            if (m->points.size() != m->next_points.size()) throw GyroflowCoreError(GyroflowCoreError::Unknown, "find_offsets_rssync: a pair's two point sets have one length");      // :128
            ts.push_back(m->timestamp_us); ts.push_back(m->next_timestamp_us);
            for (const auto &pt : m->points) { a.push_back(pt.first); a.push_back(pt.second); }
            for (const auto &pt : m->next_points) { b.push_back(pt.first); b.push_back(pt.second); }
            first.push_back((int32_t)(a.size() / 2));
        }
        range_first.push_back((int32_t)(ts.size() / 2));
        sync_points.emplace_back(in.front()->timestamp_us, in.back()->next_timestamp_us);           // :116-119
    }
    if (sync_points.empty()) return offsets;
    if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "find_offsets_rssync: no backend context for the rs-sync search");
    const double presync_radius = sync_params.search_size, initial_delay = -sync_params.initial_offset;      // :165-166
    std::vector<gfw_sync_result> results(sync_points.size());
    std::memset(results.data(), 0, sizeof(gfw_sync_result) * results.size());
    const int rc = gfw_sync_rs_search(ctx, &params, &cfg, range_first.data(), (int)sync_points.size(), ts.data(), first.data(), a.data(), b.data(), (int)(ts.size() / 2),
                                      track_timestamps_us.data(), track_wxyz.data(), (int)track_timestamps_us.size(), initial_delay / 1000.0, presync_radius / 1000.0,
                                      results.data(), nullptr, nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    const double frame_readout_time = cfg.frame_readout_time_ms / 1000.0;                           // :81
    for (size_t k = 0; k < sync_points.size(); ++k) {
        if (!results[k].found) continue;
        const double offset = results[k].value * 1000.0, d = offset - initial_delay;
        if ((d < 0.0 ? -d : d) < presync_radius * 0.9)                                              // :178
            offsets.emplace_back((double)(sync_points[k].first + sync_points[k].second) / 2.0 / 1000.0, -offset - (frame_readout_time * 1000.0 / 2.0), results[k].cost);
    }
    return offsets;
}

// ---- synchronization/estimate_pose/almeida.rs over gfw_pose_almeida: `PoseEstimator::process_detected_frames` (synchronization/mod.rs:110-167) with the Almeida
// method for ALL frame pairs in one device call, and the host part of `recalculate_gyro_data` (:269-361) that turns the rotations into the series
// find_offsets_essential takes.  `pairs`: one entry per frame pair in order; an entry without points (the optical flow found no lines) has no rotation (:141).
// The reference draws a round's points from an unseeded generator; here `seed` decides them (gfw_pose_draws).  `params`: the KernelParams undistort_points builds;
// `cfg`: sizes, rounds, samples, the inlier angle and the camera matrix (f / c of params are its f32 cast).
struct FlowPair { bool has_points = false; std::vector<std::pair<float, float>> points, next_points; };
struct PoseResult { bool has_rotation = false; double rotation[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; float quat[4] = {1, 0, 0, 0}; double euler[3] = {0, 0, 0}; int inliers = 0, round = -1; };
// Rotation3::scaled_axis: the axis of the skew part (none when its norm is not above the f64 epsilon) times acos((trace - 1) / 2)
inline std::array<double, 3> scaled_axis(const double *m) {
    const double ax = m[7] - m[5], ay = m[2] - m[6], az = m[3] - m[1];
    const double norm = std::sqrt(ax * ax + ay * ay + az * az);
    if (!(norm > 2.220446049250313e-16)) return {0.0, 0.0, 0.0};
    const double c = (m[0] + m[4] + m[8] - 1.0) / 2.0, angle = std::acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
    return {ax / norm * angle, ay / norm * angle, az / norm * angle};
}
inline std::vector<PoseResult> estimate_poses_almeida(gfw_ctx *ctx, const KernelParams &params, const gfw_pose_almeida_cfg &cfg, const std::vector<FlowPair> &pairs,
                                                      double scaled_fps, double every_nth_frame = 1.0, uint64_t seed = 0) {
    std::vector<PoseResult> out(pairs.size());
    std::vector<size_t> live;
    std::vector<int32_t> first{0}, sample_first{0};
    std::vector<float> a, b;
    for (size_t i = 0; i < pairs.size(); ++i) {
        const FlowPair &p = pairs[i];
        if (!p.has_points) continue;
        if (p.points.size() != p.next_points.size()) throw GyroflowCoreError(GyroflowCoreError::Unknown, "estimate_poses_almeida: a pair's two point sets have one length");
        for (const auto &pt : p.points) { a.push_back(pt.first); a.push_back(pt.second); }
        for (const auto &pt : p.next_points) { b.push_back(pt.first); b.push_back(pt.second); }
        first.push_back((int32_t)(a.size() / 2));
        sample_first.push_back(sample_first.back() + cfg.num_iters * (int32_t)std::min<size_t>(p.points.size(), (size_t)std::max(cfg.num_samples, 0)));
        live.push_back(i);
    }
    if (live.empty()) return out;
    if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "estimate_poses_almeida: no backend context for the pose estimation");
    const int n = (int)live.size();
    std::vector<int32_t> triples((size_t)n * (size_t)std::max(cfg.num_iters, 0) * 3 + 1), samples((size_t)sample_first.back() + 1), best((size_t)n * 2);
    std::vector<float> quats((size_t)n * 4);
    std::vector<double> rotations((size_t)n * 9);
    int rc = gfw_pose_draws(seed, first.data(), n, cfg.num_iters, cfg.num_samples, triples.data(), sample_first.data(), samples.data());
    if (rc == GFW_OK) rc = gfw_pose_almeida(ctx, &params, &cfg, first.data(), a.data(), b.data(), n, triples.data(), sample_first.data(), samples.data(),
                                            quats.data(), rotations.data(), best.data(), nullptr, nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (int k = 0; k < n; ++k) {
        PoseResult &r = out[live[(size_t)k]];
        r.has_rotation = true;
        std::copy(rotations.begin() + k * 9, rotations.begin() + k * 9 + 9, r.rotation);
        std::copy(quats.begin() + k * 4, quats.begin() + k * 4 + 4, r.quat);
        const auto rv = scaled_axis(r.rotation);
        for (int i = 0; i < 3; ++i) r.euler[i] = rv[(size_t)i] * (scaled_fps / every_nth_frame);      // :146
        r.inliers = best[(size_t)k * 2]; r.round = best[(size_t)k * 2 + 1];
    }
    return out;
}
// ---- pose methods 0 (`PoseFindEssentialMat`) and 2 (`PoseEightPoint`) of estimate_pose/mod.rs:27-36 over gfw_pose_essential: the rotation part of an essential
// matrix fitted to each pair's undistorted bearings, ALL frame pairs in one device call — for pairs whose camera also moved.  Neither OpenCV's LMedS nor ARRSAC is
// reproduced (include/gfwarp.h says what runs instead).  `pairs`, `params`, `seed` as for estimate_poses_almeida; the rounds' eight points come from
// gfw_pose_draws_k.  A pair without points, or for which no rotation is found (found = 0), has has_rotation = false; `front`: the inliers in front of both cameras.
struct PoseEssentialResult : PoseResult { int front = 0; double essential[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; };
inline std::vector<PoseEssentialResult> estimate_poses_essential(gfw_ctx *ctx, const KernelParams &params, const gfw_pose_essential_cfg &cfg, const std::vector<FlowPair> &pairs,
                                                                 double scaled_fps, double every_nth_frame = 1.0, uint64_t seed = 0) {
    std::vector<PoseEssentialResult> out(pairs.size());
    std::vector<size_t> live;
    std::vector<int32_t> first{0};
    std::vector<float> a, b;
    for (size_t i = 0; i < pairs.size(); ++i) {
        const FlowPair &p = pairs[i];
        if (!p.has_points) continue;
        if (p.points.size() != p.next_points.size()) throw GyroflowCoreError(GyroflowCoreError::Unknown, "estimate_poses_essential: a pair's two point sets have one length");
        for (const auto &pt : p.points) { a.push_back(pt.first); a.push_back(pt.second); }
        for (const auto &pt : p.next_points) { b.push_back(pt.first); b.push_back(pt.second); }
        first.push_back((int32_t)(a.size() / 2));
        live.push_back(i);
    }
    if (live.empty()) return out;
    if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "estimate_poses_essential: no backend context for the pose estimation");
    const int n = (int)live.size();
    std::vector<int32_t> octets((size_t)n * (size_t)std::max(cfg.num_iters, 0) * 8 + 1), best((size_t)n * 4);
    std::vector<float> quats((size_t)n * 4);
    std::vector<double> rotations((size_t)n * 9), essential((size_t)n * 9);
    int rc = gfw_pose_draws_k(seed, first.data(), n, cfg.num_iters, 8, octets.data());
    if (rc == GFW_OK) rc = gfw_pose_essential(ctx, &params, &cfg, first.data(), a.data(), b.data(), n, octets.data(), quats.data(), rotations.data(), essential.data(),
                                              best.data(), nullptr, nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (int k = 0; k < n; ++k) {
        PoseEssentialResult &r = out[live[(size_t)k]];
        r.has_rotation = best[(size_t)k * 4 + 3] != 0;
        std::copy(rotations.begin() + k * 9, rotations.begin() + k * 9 + 9, r.rotation);
        std::copy(essential.begin() + k * 9, essential.begin() + k * 9 + 9, r.essential);
        std::copy(quats.begin() + k * 4, quats.begin() + k * 4 + 4, r.quat);
        const auto rv = scaled_axis(r.rotation);
        for (int i = 0; i < 3; ++i) r.euler[i] = rv[(size_t)i] * (scaled_fps / every_nth_frame);      // :146
        r.inliers = best[(size_t)k * 4]; r.round = best[(size_t)k * 4 + 1]; r.front = best[(size_t)k * 4 + 2];
    }
    return out;
}
// ---- synchronization/optical_flow/opencv_pyrlk.rs:63-119 over gfw_flow_pyrlk: `OFOpenCVPyrLK::optical_flow_to` for ALL frame pairs in one device call.  `frames`:
// n u8 gray planes back to back (host memory), `pairs` (first frame, second frame); `features`: one list per frame, or empty for the grid points of
// opencv_dis.rs:62-119 (computed on the device).  One FlowPair per pair, in feature order; has_points only with at least 10 kept points (:107) — what
// estimate_poses_almeida takes.
inline std::vector<FlowPair> optical_flow_pyrlk(gfw_ctx *ctx, const uint8_t *frames, int n_frames, int width, int height, int stride, const std::vector<std::pair<int, int>> &pairs,
                                                const std::vector<std::vector<std::pair<float, float>>> &features = {}) {
    std::vector<FlowPair> out(pairs.size());
    if (pairs.empty()) return out;
    if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "optical_flow_pyrlk: no backend context for the optical flow");
    const bool grid = features.empty();
    if (!grid && (int)features.size() != n_frames) throw GyroflowCoreError(GyroflowCoreError::Unknown, "optical_flow_pyrlk: one feature list per frame");
    gfw_flow_pyrlk_cfg cfg = {width, height, stride, grid ? 1 : 0, 0};
    std::vector<int32_t> pf, first{0};
    std::vector<float> feats;
    for (const auto &p : pairs) { pf.push_back(p.first); pf.push_back(p.second); }
    for (const auto &f : features) { for (const auto &pt : f) { feats.push_back(pt.first); feats.push_back(pt.second); } first.push_back((int32_t)(feats.size() / 2)); }
    size_t raw = 0;
    const int step = width >= 15 ? width / 15 : 1;
    const size_t nodes = (size_t)((width + step - 1) / step) * (size_t)((height + step - 1) / step);
    for (const auto &p : pairs) raw += grid ? nodes : (p.first >= 0 && p.first < n_frames ? features[(size_t)p.first].size() : 0);
    std::vector<float> next(raw * 2 + 2), a(raw * 2 + 2), b(raw * 2 + 2);
    std::vector<uint8_t> status(raw + 1);
    std::vector<int32_t> pair_first(pairs.size() + 1);
    feats.push_back(0.0f);
    const int rc = gfw_flow_pyrlk(ctx, &cfg, frames, 0, n_frames, pf.data(), (int)pairs.size(), grid ? nullptr : first.data(), grid ? nullptr : feats.data(),
                                  next.data(), status.data(), nullptr, nullptr, nullptr, pair_first.data(), a.data(), b.data(), 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (pair_first[p + 1] - pair_first[p] < 10) continue;
        out[p].has_points = true;
        for (int k = pair_first[p]; k < pair_first[p + 1]; ++k) { out[p].points.push_back({a[(size_t)k * 2], a[(size_t)k * 2 + 1]}); out[p].next_points.push_back({b[(size_t)k * 2], b[(size_t)k * 2 + 1]}); }
    }
    return out;
}
// ---- synchronization/optical_flow/opencv_dis.rs over gfw_flow_dis: `OFOpenCVDis::optical_flow_to` (the reference's DEFAULT method 2) for ALL frame pairs in one
// device call: the DIS dense flow with the parameters of DISOpticalFlow_PRESET_FAST read at the grid points of :62-119.  `variational_iters`: the fixed-point
// iterations of the preset's variational refinement on every level (gfw_flow_dis_refined, its other parameters at their defaults); the reference's preset is 5, the
// default here stays 0, the unrefined gfw_flow_dis.  `frames`: n u8 gray planes back to back (host memory), `pairs` (first frame, second frame); finest_scale 2 as the reference, or 1.  One FlowPair per
// pair: every node the grid keeps in the first frame and where the flow takes it, unfiltered (:113-117); has_points only with at least 10 nodes (:126) — what
// estimate_poses_almeida takes.
inline std::vector<FlowPair> optical_flow_dis(gfw_ctx *ctx, const uint8_t *frames, int n_frames, int width, int height, int stride, const std::vector<std::pair<int, int>> &pairs,
                                              int finest_scale = 2, int variational_iters = 0) {
    std::vector<FlowPair> out(pairs.size());
    if (pairs.empty()) return out;
    if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "optical_flow_dis: no backend context for the optical flow");
    gfw_flow_dis_cfg cfg = {width, height, stride, finest_scale, 0, 0};
    std::vector<int32_t> pf;
    for (const auto &p : pairs) { pf.push_back(p.first); pf.push_back(p.second); }
    const int step = width >= 15 ? width / 15 : 1;
    const size_t room = pairs.size() * (size_t)((width + step - 1) / step) * (size_t)((height + step - 1) / step);
    std::vector<float> a(room * 2 + 2), b(room * 2 + 2);
    std::vector<int32_t> pair_first(pairs.size() + 1);
    const gfw_flow_varref_cfg ref = {variational_iters, 5, 20.0f, 5.0f, 10.0f, 1.6f, {0, 0}};
    const int rc = variational_iters == 0
        ? gfw_flow_dis(ctx, &cfg, frames, 0, n_frames, pf.data(), (int)pairs.size(), nullptr, nullptr, nullptr, pair_first.data(), a.data(), b.data(), 0)
        : gfw_flow_dis_refined(ctx, &cfg, &ref, frames, 0, n_frames, pf.data(), (int)pairs.size(), nullptr, nullptr, nullptr, pair_first.data(), a.data(), b.data(), 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (pair_first[p + 1] - pair_first[p] < 10) continue;
        out[p].has_points = true;
        for (int k = pair_first[p]; k < pair_first[p + 1]; ++k) { out[p].points.push_back({a[(size_t)k * 2], a[(size_t)k * 2 + 1]}); out[p].next_points.push_back({b[(size_t)k * 2], b[(size_t)k * 2 + 1]}); }
    }
    return out;
}
// ---- synchronization/optical_flow/opencv_pyrlk.rs:25-42 over gfw_corners_shi_tomasi: `OFOpenCVPyrLK::detect_features` for ALL frames in one device call with the
// reference's parameters, good_features_to_track(img, 200, 0.01, 10.0, ..).  `frames`: n u8 gray planes back to back (host memory).  One list per frame, in pick
// order: exactly the `features` of optical_flow_pyrlk.
inline std::vector<std::vector<std::pair<float, float>>> detect_features_pyrlk(gfw_ctx *ctx, const uint8_t *frames, int n_frames, int width, int height, int stride) {
    std::vector<std::vector<std::pair<float, float>>> out((size_t)(n_frames > 0 ? n_frames : 0));
    if (n_frames == 0) return out;
    if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "detect_features_pyrlk: no backend context for the corner detection");
    gfw_corners_cfg cfg = {width, height, stride, 200, 0.01f, 10.0f, 0, 0};
    std::vector<float> corners(out.size() * 200 * 2 + 2);
    std::vector<int32_t> counts(out.size() + 1);
    const int rc = gfw_corners_shi_tomasi(ctx, &cfg, frames, 0, n_frames, corners.data(), nullptr, counts.data(), nullptr, nullptr, 0);
    if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
    for (size_t f = 0; f < out.size(); ++f)
        for (int k = 0; k < counts[f]; ++k) out[f].push_back({corners[(f * 200 + (size_t)k) * 2], corners[(f * 200 + (size_t)k) * 2 + 1]});
    return out;
}
// `results`: every analysed frame's timestamp_us -> its euler, or nullopt without a rotation (a sample sits midway to the NEXT analysed frame, :312-315);
// final_pass interpolates a missing rotation linearly between its neighbours that have one (:284-305); lpf > 0 (Hz) runs gfw_lowpass_gyro (:349-357)
inline std::map<int64_t, TimeIMU> estimated_gyro(const std::map<int64_t, std::optional<std::array<double, 3>>> &results, double fps, double lpf = 0.0, bool final_pass = false) {
    std::map<int64_t, TimeIMU> gyro;
    for (auto it = results.begin(); it != results.end(); ++it) {
        std::optional<std::array<double, 3>> eul = it->second;
        if (final_pass && !eul) {
            auto prev = results.end(), next = results.end();
            for (auto p = it; p != results.begin();) { --p; if (p->second) { prev = p; break; } }
            for (auto p = it; p != results.end(); ++p) if (p->second) { next = p; break; }
            if (prev != results.end() && next != results.end()) {
                const double ratio = (double)(it->first - prev->first) / (double)(next->first - prev->first);
                std::array<double, 3> e;
                for (size_t i = 0; i < 3; ++i) e[i] = (*prev->second)[i] + ((*next->second)[i] - (*prev->second)[i]) * ratio;
                eul = e;
            }
        }
        if (!eul) continue;
        double ts = (double)it->first / 1000.0;
        const auto nx = std::next(it);
        if (nx != results.end()) ts += ((double)nx->first / 1000.0 - ts) / 2.0;
        TimeIMU x;
        x.timestamp_ms = ts; x.has_gyro = true;
        const double pi = 3.14159265358979323846;
        x.gyro[0] = (*eul)[1] * 180.0 / pi; x.gyro[1] = (*eul)[0] * 180.0 / pi; x.gyro[2] = (*eul)[2] * 180.0 / pi;      // x and y swapped (:322-326)
        gyro[(int64_t)std::round(ts * 1000.0)] = x;
    }
    if (lpf > 0.0 && fps > 0.0 && !gyro.empty()) {
        std::vector<double> xyz;
        for (const auto &kv : gyro) for (int a = 0; a < 3; ++a) xyz.push_back(kv.second.gyro[a]);
        const int rc = gfw_lowpass_gyro(lpf, fps, xyz.data(), nullptr, (int)gyro.size());               // a refusal is logged and ignored by the reference
        if (rc < 0) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
        size_t i = 0;
        for (auto &kv : gyro) { for (int a = 0; a < 3; ++a) kv.second.gyro[a] = xyz[i * 3 + (size_t)a]; ++i; }
    }
    return gyro;
}

// OptimSync (optimsync.rs:10-226): where in a clip to sync, decided before any optical flow (lib.rs:2054-2060).  `make` is OptimSync::new — the gyro resampled at its
// average rate on the host (gfw_optim_resample; nullopt without samples, as the reference's None) — and `run` is OptimSync::run in ONE device call
// (gfw_sync_optim_points): (points in ms, the rank of every window before the masks, ratio = 16 / sample_rate).
struct OptimSync {
    double sample_rate = 0.0;
    std::array<std::vector<double>, 3> gyro;

    static std::optional<OptimSync> make(const std::vector<TimeIMU> &raw_imu) {
        if (raw_imu.empty()) return std::nullopt;
        std::vector<double> ts(raw_imu.size()), xyz(raw_imu.size() * 3);
        std::vector<uint8_t> has(raw_imu.size());
        for (size_t i = 0; i < raw_imu.size(); ++i) {
            ts[i] = raw_imu[i].timestamp_ms; has[i] = raw_imu[i].has_gyro ? 1 : 0;
            for (int a = 0; a < 3; ++a) xyz[i * 3 + a] = raw_imu[i].gyro[a];
        }
        OptimSync o;
        int64_t n = 0;
        int rc = gfw_optim_resample(ts.data(), xyz.data(), has.data(), (int)raw_imu.size(), nullptr, 0, &n, &o.sample_rate);
        if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
        std::vector<double> flat((size_t)n * 3);
        if (n) rc = gfw_optim_resample(ts.data(), xyz.data(), has.data(), (int)raw_imu.size(), flat.data(), n, &n, &o.sample_rate);
        if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
        for (int a = 0; a < 3; ++a) o.gyro[a].assign(flat.begin() + (size_t)a * (size_t)n, flat.begin() + (size_t)(a + 1) * (size_t)n);
        return o;
    }

    std::tuple<std::vector<double>, std::vector<float>, double> run(gfw_ctx *ctx, size_t target_sync_points, const std::vector<std::pair<double, double>> &trim_ranges_s) const {
        if (!ctx) throw GyroflowCoreError(GyroflowCoreError::Unknown, "OptimSync::run: no backend context for the sync point search");
        const size_t n = gyro[0].size();
        std::vector<double> flat(n * 3), trim(trim_ranges_s.size() * 2), points(std::max<size_t>(target_sync_points, 1));
        for (int a = 0; a < 3; ++a) std::copy(gyro[a].begin(), gyro[a].end(), flat.begin() + (size_t)a * n);
        for (size_t i = 0; i < trim_ranges_s.size(); ++i) { trim[2 * i] = trim_ranges_s[i].first; trim[2 * i + 1] = trim_ranges_s[i].second; }
        std::vector<float> rank(n / 16 + 2);
        int32_t n_points = 0;
        double ratio = 0.0;
        int rc = gfw_sync_optim_points(ctx, flat.data(), (int64_t)n, sample_rate, (int)std::min<size_t>(target_sync_points, (size_t)1 << 30), trim.data(), (int)trim_ranges_s.size(),
                                       points.data(), &n_points, rank.data(), nullptr, &ratio, 0);
        if (rc != GFW_OK) throw GyroflowCoreError(GyroflowCoreError::from_code(rc), gfw_last_error());
        const double fft = std::floor(sample_rate + 0.5);
        const size_t n_windows = (double)n < fft ? 0 : (n - (size_t)fft) / 16 + 1;                  // windows(fft_size).step_by(16), fft_size = sample_rate.round()
        points.resize((size_t)n_points); rank.resize(n_windows);
        return {points, rank, ratio};
    }
};

}  // namespace gyroflow
