// gfw_zoom_host.h — host only: what gfw_zoom_fovs / gfw_zoom_fovs_stab stage for the kernels of gfw_zoom.hip, and the host half of the adaptive zoom
// (gfw_zoom_smooth).  Included behind gfw_zoom.h (GfwZoomArgs) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's translation unit sees
// it, it calls nothing of HIP and reports no errors (the entry points validate).
#pragma once
#include <math.h>
#include <string.h>
#include <vector>
#include "gfw_matrices_host.h"

// The staged block: frames, caller-given rotations, the stabiliser table and its control points, a (first double, length) mesh reference per frame, the clip's distinct
// meshes back to back.  A frame that names the array and length of the frame before shares that frame's copy.
struct GfwZoomLayout { size_t o_frames, o_rot, o_ref, o_mesh, total; GfwStabTable stab; };
inline bool gfw_zoom_mesh_repeats(const double *const *meshes, const size_t *mesh_lens, int i) { return i && meshes[i] == meshes[i - 1] && mesh_lens[i] == mesh_lens[i - 1]; }
inline size_t gfw_zoom_mesh_doubles(const double *const *meshes, const size_t *mesh_lens, int n_frames) {
    size_t n = 0;
    for (int i = 0; i < n_frames; ++i) if (mesh_lens[i] && !gfw_zoom_mesh_repeats(meshes, mesh_lens, i)) n += mesh_lens[i];
    return n;
}
inline GfwZoomLayout gfw_zoom_layout(int n_frames, bool rotations, bool stabs, size_t point_bytes, bool meshes, size_t mesh_doubles) {
    static_assert(sizeof(gfw_zoom_frame) % 8 == 0 && sizeof(GfwStab) % 8 == 0, "the staged block keeps its doubles aligned");
    BlockLayout L;
    GfwZoomLayout Z;
    Z.o_frames = L.add(sizeof(gfw_zoom_frame) * (size_t)n_frames);
    Z.o_rot = L.add(rotations ? sizeof(float) * 9 * (size_t)n_frames : 0);
    Z.stab = gfw_stab_table_layout(L, stabs ? n_frames : 0, stabs ? point_bytes : 0);
    Z.o_ref = L.add(meshes ? sizeof(int32_t) * 2 * (size_t)n_frames : 0);
    Z.o_mesh = L.add(meshes ? sizeof(double) * mesh_doubles : 0);
    Z.total = L.total;
    return Z;
}
// Fills the block at (h, d) and the argument block's input pointers (NULL tables stay NULL: the plain instantiations are launched)
inline void gfw_zoom_fill(const GfwZoomLayout &Z, const gfw_zoom_frame *frames, int n_frames, const float *rotations, const gfw_frame_stab *const *stabs,
                          const double *const *meshes, const size_t *mesh_lens, char *h, const char *d, GfwZoomArgs &A) {
    memcpy(h + Z.o_frames, frames, sizeof(gfw_zoom_frame) * (size_t)n_frames);
    A.frames = (const gfw_zoom_frame *)(d + Z.o_frames);
    A.rotations = nullptr; A.stabs = nullptr; A.mesh_ref = nullptr; A.mesh_data = nullptr;
    if (rotations) { memcpy(h + Z.o_rot, rotations, sizeof(float) * 9 * (size_t)n_frames); A.rotations = (const float *)(d + Z.o_rot); }
    if (stabs) A.stabs = gfw_stab_table_fill(Z.stab, stabs, nullptr, n_frames, h, d);
    if (meshes) {
        int32_t *ref = (int32_t *)(h + Z.o_ref);
        double *hm = (double *)(h + Z.o_mesh);
        size_t at = 0, first = 0;
        for (int i = 0; i < n_frames; ++i) {
            if (!mesh_lens[i]) { ref[i * 2] = 0; ref[i * 2 + 1] = 0; continue; }
            if (!gfw_zoom_mesh_repeats(meshes, mesh_lens, i)) { first = at; memcpy(hm + at, meshes[i], mesh_lens[i] * sizeof(double)); at += mesh_lens[i]; }
            ref[i * 2] = (int32_t)first; ref[i * 2 + 1] = (int32_t)mesh_lens[i];
        }
        A.mesh_ref = (const int32_t *)(d + Z.o_ref); A.mesh_data = (const double *)(d + Z.o_mesh);
    }
}
// FovIterative::new (fov_iterative.rs:74-80), f32
inline void gfw_zoom_search_args(const gfw_zoom_search &search, GfwZoomArgs &A) {
    A.horizontal = search.horizontal_readout;
    A.w = (float)search.width; A.h = (float)search.height; A.margin = search.fov_algorithm_margin;
    const float ratio = (float)search.width / (float)(search.org_output_width > 1 ? search.org_output_width : 1);                  // .max(1)
    const float out_dim0 = (float)search.org_output_width * ratio, out_dim1 = (float)search.org_output_height * ratio;
    A.out_dim0 = out_dim0; A.inv_aspect = out_dim1 / out_dim0;
    A.readout_dim = search.horizontal_readout ? search.width : search.height;
}

// Adaptive zoom, second half, on the host: zooming/mod.rs:55-68 and zoom_dynamic.rs in f64, the reference's operation order.
inline int zoom_frames_per_window(double window, double fps) {               // zoom_dynamic.rs:84-90 (`as usize` saturates; NaN -> 0)
    const double v = floor(window * fps);
    long long frames = !(v == v) || v <= 0.0 ? 0 : (v >= 1e9 ? 1000000000LL : (long long)v);
    if (frames % 2 == 0) frames += 1;
    return (int)frames;
}
inline std::vector<double> zoom_pad_edge(const std::vector<double> &a, size_t before, size_t after) {       // :119-131
    std::vector<double> out(a.size() + before + after, 0.0);
    const double first = a.empty() ? 0.0 : a.front(), last = a.empty() ? 0.0 : a.back();
    for (size_t i = 0; i < a.size(); ++i) out[before + i] = a[i];
    for (size_t i = 0; i < before; ++i) out[i] = first;
    for (size_t i = before + a.size(); i < out.size(); ++i) out[i] = last;
    return out;
}
inline std::vector<double> zoom_envelope_follower(const std::vector<double> &a, double alpha) {             // :170-194 with a constant alpha
    const size_t n = a.size();
    std::vector<double> rev(n), out(n);
    if (!n) return out;
    double q = a[n - 1];
    for (size_t k = 0; k < n; ++k) { const double x = a[n - 1 - k]; q = fmin(x, x * alpha + q * (1.0 - alpha)); rev[k] = q; }      // smoothed_rev, in reversed order
    q = rev[n - 1];
    for (size_t k = 0; k < n; ++k) { const double x = rev[n - 1 - k]; q = fmin(x, x * alpha + q * (1.0 - alpha)); out[k] = q; }
    return out;
}
// gfw_zoom_smooth behind its validation: n >= 1
inline void gfw_zoom_smooth_host(const double *fov_minimal, int n, double adaptive_zoom_window, double scaled_fps, int method,
                                 const double *trim_ranges, int n_ranges, double *fovs_out, double *fov_minimal_out) {
    std::vector<double> v(fov_minimal, fov_minimal + n);
    if (n_ranges > 0) {                                                      // fov_iterative.rs:59-69
        const double l = (double)(n - 1);
        double max_fov = v[0];
        for (int i = 1; i < n; ++i) max_fov = fmax(max_fov, v[i]);
        for (int i = 0; i < n; ++i) {
            bool within = false;
            for (int r = 0; r < n_ranges && !within; ++r) {
                const double lo = floor(l * trim_ranges[r * 2]), hi = ceil(l * trim_ranges[r * 2 + 1]);
                const double lo_u = !(lo == lo) || lo <= 0.0 ? 0.0 : lo, hi_u = !(hi == hi) || hi <= 0.0 ? 0.0 : hi;              // `as usize`
                within = (double)i >= lo_u && (double)i <= hi_u;
            }
            if (!within) v[i] = max_fov;
        }
    }
    if (fov_minimal_out) for (int i = 0; i < n; ++i) fov_minimal_out[i] = v[i];
    if (adaptive_zoom_window < -0.9) {                                       // static zoom (mod.rs:55-61)
        double m = v[0];
        for (int i = 1; i < n; ++i) m = fmin(m, v[i]);
        for (int i = 0; i < n; ++i) fovs_out[i] = m;
    } else if (adaptive_zoom_window > 0.0001) {                              // dynamic zoom (zoom_dynamic.rs:56-79)
        if (method == 1) {
            const double first_pass_alpha = 1.0 - exp(-(1.0 / scaled_fps) / adaptive_zoom_window);
            const double second_pass_alpha = 1.0 - exp(-(1.0 / scaled_fps) / 0.2);
            v = zoom_envelope_follower(zoom_envelope_follower(v, first_pass_alpha), second_pass_alpha);
        } else {
            const int frames = zoom_frames_per_window(adaptive_zoom_window, scaled_fps);
            const size_t half = (size_t)(frames / 2);
            const std::vector<double> pad = zoom_pad_edge(v, half, half);
            std::vector<double> mn((size_t)n);
            for (int i = 0; i < n; ++i) { double m = pad[i]; for (int k = 1; k < frames; ++k) m = fmin(m, pad[(size_t)i + k]); mn[i] = m; }        // min_rolling
            const std::vector<double> mpad = zoom_pad_edge(mn, half, half);
            std::vector<double> g((size_t)frames);                           // gaussian_window_normalized(frames, frames / 6)
            const double std_ = (double)frames / 6.0, sig2 = 2.0 * (std_ * std_);
            double sum = 0.0;
            for (int k = 0; k < frames; ++k) { const long long x = (long long)k - frames / 2; g[k] = exp(-((double)(x * x)) / sig2); }
            for (int k = 0; k < frames; ++k) sum += g[k];
            for (int k = 0; k < frames; ++k) g[k] /= sum;
            for (int i = 0; i < n; ++i) { double s = 0.0; for (int k = 0; k < frames; ++k) s += mpad[(size_t)i + k] * g[k]; v[i] = s; }          // convolve
        }
        for (int i = 0; i < n; ++i) fovs_out[i] = v[i];
    } else {
        for (int i = 0; i < n; ++i) fovs_out[i] = 1.0;                       // disabled
    }
}
