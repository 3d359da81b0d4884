// gfw_points.h — the inverse point map of `undistort_points` (cpu_undistort.rs:652-858) as a device function: what gfw_points_kernel
// (gfw_kernels.hip) runs per point and what the zoom search (gfw_zoom.hip) runs per outline point.
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_fastmath.h"

// undistort_points' lens-correction branch (cpu_undistort.rs:785-851): Newton solve of amount*o + (1-amount)*R(o) = pt,
// R = the render's forward map (digital undistort -> /out_f -> radial undistort -> refraction -> *out_f), :804-826.
struct GfwLc { float out_c0, out_c1, out_f0, out_f1, amount, factor, fov; };
template <int MODEL>
__device__ inline float2 gfw_lc_r_of(const GfwLc &L, float o0, float o1, const gfw_kernel_params &P, const GfwCommon &C) {
    float q0 = o0, q1 = o1;
    if (C.digital != GFW_MODEL_NONE) {
        const float uz0 = (q0 - L.out_c0) * L.fov + L.out_c0, uz1 = (q1 - L.out_c1) * L.fov + L.out_c1;
        const GfwPt d = gfw_lens::digital_undistort(C.digital, uz0, uz1, P);
        if (d.ok) { q0 = (d.x - L.out_c0) / L.fov + L.out_c0; q1 = (d.y - L.out_c1) / L.fov + L.out_c1; }
    }
    float n0 = (q0 - L.out_c0) / L.out_f0, n1 = (q1 - L.out_c1) / L.out_f1;
    const GfwPt d = gfw_lens::undistort<MODEL>(C.model, n0, n1, P, C);
    if (d.ok) { n0 = d.x; n1 = d.y; }
    if (P.light_refraction_coefficient != 1.0f && P.light_refraction_coefficient > 0.0f) {
        const float r = sqrtf(n0 * n0 + n1 * n1);
        if (r != 0.0f) {
            const float sin_theta_d = (r / sqrtf(1.0f + r * r)) / P.light_refraction_coefficient;
            const float r_d = sin_theta_d / sqrtf(1.0f - sin_theta_d * sin_theta_d);
            const float sc = r_d / r;
            n0 = n0 * sc; n1 = n1 * sc;
        }
    }
    return float2{(n0 * L.out_f0) + L.out_c0, (n1 * L.out_f1) + L.out_c1};
}
__device__ __forceinline__ bool gfw_finite(float x) { return fabsf(x) < __builtin_inff(); }   // false for inf and NaN
template <int MODEL>
__device__ inline float2 gfw_lc_solve(const GfwLc &L, float p0, float p1, const gfw_kernel_params &P, const GfwCommon &C) {
    float inv0, inv1;
    {
        const float n0 = (p0 - L.out_c0) / L.out_f0, n1 = (p1 - L.out_c1) / L.out_f1;
        float d0, d1;
        gfw_lens::distort<MODEL>(C.model, n0, n1, 1.0f, P, C, d0, d1);
        inv0 = (d0 * L.out_f0) + L.out_c0; inv1 = (d1 * L.out_f1) + L.out_c1;
        if (C.digital != GFW_MODEL_NONE) {
            const float uz0 = (inv0 - L.out_c0) * L.fov + L.out_c0, uz1 = (inv1 - L.out_c1) * L.fov + L.out_c1;
            float dd0, dd1;
            gfw_lens::digital_distort(C.digital, uz0, uz1, P, dd0, dd1);
            inv0 = (dd0 - L.out_c0) / L.fov + L.out_c0; inv1 = (dd1 - L.out_c1) / L.fov + L.out_c1;
        }
    }
    float o0 = p0, o1 = p1;
    if (gfw_finite(inv0) && gfw_finite(inv1)) { o0 = inv0 * L.factor + p0 * L.amount; o1 = inv1 * L.factor + p1 * L.amount; }
    #pragma unroll 1
    for (int it = 0; it < 10; ++it) {
        const float2 r = gfw_lc_r_of<MODEL>(L, o0, o1, P, C);
        const float g0 = L.amount * o0 + L.factor * r.x - p0, g1 = L.amount * o1 + L.factor * r.y - p1;
        if (fabsf(g0) < 0.02f && fabsf(g1) < 0.02f) break;
        const float eps = 1.0f;
        const float2 rx = gfw_lc_r_of<MODEL>(L, o0 + eps, o1, P, C);
        const float2 ry = gfw_lc_r_of<MODEL>(L, o0, o1 + eps, P, C);
        const float j11 = L.amount + L.factor * (rx.x - r.x) / eps, j21 = L.factor * (rx.y - r.y) / eps;
        const float j12 = L.factor * (ry.x - r.x) / eps,            j22 = L.amount + L.factor * (ry.y - r.y) / eps;
        const float det = j11 * j22 - j12 * j21;
        if (!gfw_finite(det) || fabsf(det) < 1e-9f) break;
        const float dx = ( j22 * g0 - j12 * g1) / det;
        const float dy = (-j21 * g0 + j11 * g1) / det;
        if (!gfw_finite(dx) || !gfw_finite(dy)) break;
        o0 = o0 - dx; o1 = o1 - dy;
    }
    return float2{o0, o1};
}

// One point (x, y) of the source image -> stabilised output coordinate.  rot: the point's `new_k * R` (9 f32, row-major); shifts: its 6 floats
// (sx, sy, cos, sin, ox, oy) or nullptr; mesh: the f64 lens mesh or mesh_len = 0; lens_correction_amount / fov: the blend's (:683-692).
template <int MODEL>
__device__ __forceinline__ float2 gfw_point_map(const gfw_kernel_params &P, const GfwCommon &C, float x, float y, const float *rot, const float *shifts,
                                                const double *mesh, int mesh_len, float lens_correction_amount, float fov) {
    if (P.input_horizontal_stretch > 0.001f) x *= P.input_horizontal_stretch;                 // :704-705
    if (P.input_vertical_stretch   > 0.001f) y *= P.input_vertical_stretch;
    if (C.digital != GFW_MODEL_NONE) {                                                         // :707-712
        const GfwPt d = gfw_lens::digital_undistort(C.digital, x, y, P);
        if (d.ok) { x = d.x; y = d.y; }
    }
    if (mesh_len > 0) {
        const double *md = mesh;
        if (md[0] > 0.0 && md[gfw_mesh::d2us(md[0])] > 0.0) {                                  // :715-738
            const int64_t o = gfw_mesh::d2us(md[0]);
            const double ms1 = md[4];
            const float or0 = (float)md[5], or1 = (float)md[6], cs0 = (float)md[7], cs1 = (float)md[8];
            const double grid = ms1 / 8.0;
            x = gfw_map_coord(x, 0.0f, (float)P.width,  or0, or0 + cs0);
            y = gfw_map_coord(y, 0.0f, (float)P.height, or1, or1 + cs1);
            const int64_t idx = gfw_mesh::d2us(fmin(fmax(floor((double)y / grid), 0.0), 7.0));
            const double delta = (double)y - grid * (double)idx;
            x += (float)(md[o + 4 + idx * 2 + 0] * delta);
            y += (float)(md[o + 4 + idx * 2 + 1] * delta);
            for (int64_t j = 0; j < idx; ++j) {
                x += (float)(md[o + 4 + j * 2 + 0] * grid);
                y += (float)(md[o + 4 + j * 2 + 1] * grid);
            }
            x = gfw_map_coord(x, or0, or0 + cs0, 0.0f, (float)P.width);
            y = gfw_map_coord(y, or1, or1 + cs1, 0.0f, (float)P.height);
        }
        if (md[0] > 10.0) {                                                                    // :740-752
            const double ms0 = md[3], ms1 = md[4];
            const float or0 = (float)md[5], or1 = (float)md[6], cs0 = (float)md[7], cs1 = (float)md[8];
            x = gfw_map_coord(x, 0.0f, (float)P.width,  or0, or0 + cs0);
            y = gfw_map_coord(y, 0.0f, (float)P.height, or1, or1 + cs1);
            const int nx = (int)gfw_mesh::d2us(md[1]), ny = (int)gfw_mesh::d2us(md[2]);
            const double nxp = gfw_mesh::bivariate(nx, ny, ms0, ms1, md, 0, (double)x, (double)y);
            const double nyp = gfw_mesh::bivariate(nx, ny, ms0, ms1, md, 1, (double)x, (double)y);
            x = gfw_map_coord((float)nxp, or0, or0 + cs0, 0.0f, (float)P.width);
            y = gfw_map_coord((float)nyp, or1, or1 + cs1, 0.0f, (float)P.height);
        }
    }
    const float c0 = P.c[0], c1 = P.c[1];
    if (shifts) {                                                                            // :754-763
        const float *s = shifts;
        x = x - c0 - s[4] + s[0];
        y = y - c1 - s[5] + s[1];
        x = s[2] * x - s[3] * y + c0;
        y = s[3] * x + s[2] * y + c1;                        // the reference rotates y with the already-rotated x
    }
    const float pwx = (x - c0) / P.f[0], pwy = (y - c1) / P.f[1];                              // :765
    const GfwPt pt = gfw_lens::undistort<MODEL>(C.model, pwx, pwy, P, C);
    float2 o = float2{-1000000.0f, -1000000.0f};                                               // :855
    if (pt.ok) {
        float ptx = pt.x, pty = pt.y;
        if (P.light_refraction_coefficient != 1.0f && P.light_refraction_coefficient > 0.0f) { // :770-779
            const float rr = sqrtf(ptx * ptx + pty * pty);
            if (rr != 0.0f) {
                const float sin_theta_d = (rr / sqrtf(1.0f + rr * rr)) / P.light_refraction_coefficient;
                const float r_d = sin_theta_d / sqrtf(1.0f - sin_theta_d * sin_theta_d);
                const float factor = r_d / rr;
                ptx *= factor; pty *= factor;
            }
        }
        const float *r = rot;                                                                  // :782-783 (nalgebra gemv: column axpy)
        const float pr0 = ((r[0] * ptx) + r[1] * pty) + r[2];
        const float pr1 = ((r[3] * ptx) + r[4] * pty) + r[5];
        const float pr2 = ((r[6] * ptx) + r[7] * pty) + r[8];
        o = float2{pr0 / pr2, pr1 / pr2};
        if (lens_correction_amount < 1.0f) {                                                 // :683-692, :785-851
            GfwLc L;
            L.out_c0 = (float)P.output_width / 2.0f; L.out_c1 = (float)P.output_height / 2.0f;
            L.amount = lens_correction_amount;
            L.factor = fmaxf(1.0f - L.amount, 0.001f);
            L.out_f0 = P.f[0] / fov / L.factor; L.out_f1 = P.f[1] / fov / L.factor;
            L.fov = fov;
            o = gfw_lc_solve<MODEL>(L, o.x, o.y, P, C);
        }
    }
    return o;
}

// gfw_point_map without shifts, without a mesh and with lens_correction_amount 1.0, in two halves — the same operations in the same order, so the halves composed
// equal it to the bit: the sync search (gfw_sync.hip) runs the first once per point and the second once per candidate.  (gfw_point_map itself is not built from
// them: its callers' register allocation moves when it is.)
// First half — everything in front of the rotation (:704-712, :765-779): the stretches, the digital lens, (x - c) / f, the lens inverse, the refraction -> the
// ray (ptx, pty); false where the lens inverse is None.
template <int MODEL>
__device__ __forceinline__ bool gfw_point_ray(const gfw_kernel_params &P, const GfwCommon &C, float x, float y, float &ptx, float &pty) {
    if (P.input_horizontal_stretch > 0.001f) x *= P.input_horizontal_stretch;
    if (P.input_vertical_stretch   > 0.001f) y *= P.input_vertical_stretch;
    if (C.digital != GFW_MODEL_NONE) {
        const GfwPt d = gfw_lens::digital_undistort(C.digital, x, y, P);
        if (d.ok) { x = d.x; y = d.y; }
    }
    const float pwx = (x - P.c[0]) / P.f[0], pwy = (y - P.c[1]) / P.f[1];
    const GfwPt pt = gfw_lens::undistort<MODEL>(C.model, pwx, pwy, P, C);
    ptx = pt.x; pty = pt.y;
    if (pt.ok && P.light_refraction_coefficient != 1.0f && P.light_refraction_coefficient > 0.0f) {
        const float rr = sqrtf(ptx * ptx + pty * pty);
        if (rr != 0.0f) {
            const float sin_theta_d = (rr / sqrtf(1.0f + rr * rr)) / P.light_refraction_coefficient;
            const float r_d = sin_theta_d / sqrtf(1.0f - sin_theta_d * sin_theta_d);
            const float factor = r_d / rr;
            ptx *= factor; pty *= factor;
        }
    }
    return pt.ok;
}
// Second half — the ray through the point's `new_k * R` (rot: 9 f32, row-major; :782-783, nalgebra gemv: column axpy)
__device__ __forceinline__ float2 gfw_point_project(float ptx, float pty, const float *rot) {
    const float *r = rot;
    const float pr0 = ((r[0] * ptx) + r[1] * pty) + r[2];
    const float pr1 = ((r[3] * ptx) + r[4] * pty) + r[5];
    const float pr2 = ((r[6] * ptx) + r[7] * pty) + r[8];
    return float2{pr0 / pr2, pr1 / pr2};
}
