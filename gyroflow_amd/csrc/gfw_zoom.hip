// gfw_zoom.hip — adaptive zoom: FovIterative::find_fov (src/core/zooming/fov_iterative.rs:91-134) for every frame of a clip in one launch.
//
// The reference runs it under rayon on the host, once per frame after every change of smoothing, lens or sync: the outline of the source frame is mapped through
// undistort_points_with_rolling_shutter (cpu_undistort.rs:636-641), the largest centred rectangle of the output's aspect is fitted inside it (nearest_edge), and the
// three outline points around the nearest one are refined up to four times.  Frames do not depend on each other, so here a frame is a workgroup — one wave: its lanes map the
// 120 outline points (two points per lane; the f64 slerp of a rolling-shutter point and, with lens_correction_amount < 1, the Newton inverse of the blend dominate),
// park them in LDS, and lane 0 walks them in index order — nearest_edge is a sequential f32 fold whose result depends on the order (`ap.1 / inv_aspect` and
// `ap.0 * inv_aspect` do not round alike), and a few hundred steps per frame are nothing beside the lens inverses.  The refinement rounds map 63 points each (one pass of the
// wave) and are restated AS WRITTEN — see gfw_zoom_rounds.  The frame's descriptor is uniform across the workgroup (scalar loads).
// Control flow around the barriers is workgroup-uniform: the round's outcome travels through LDS.
#include <hip/hip_runtime.h>
#include "gfw_zoom.h"
#include "gfw_points.h"
#include "gfw_quat.h"
#include "gfw_spline.h"

#ifndef GFW_ZOOM_MESH_LDS
#define GFW_ZOOM_MESH_LDS 0         // 1: a frame's mesh is staged in LDS instead of read from global memory (the A/B of profiles/zoom_search_stab.txt)
#endif

// points_around_rect(w, h, 31, 31)[i] (fov_iterative.rs:154-175): f32 as written — `i as f32 * wstep`, the margin added afterwards
__device__ __forceinline__ float2 gfw_zoom_rect_point(int i, float w, float h, float margin) {
    w -= margin * 2.0f; h -= margin * 2.0f;
    const float wstep = w / 30.0f, hstep = h / 30.0f;
    float x, y;
    if (i < 30) { x = (float)i * wstep; y = 0.0f; }
    else if (i < 60) { x = w; y = (float)(i - 30) * hstep; }
    else if (i < 90) { x = (float)(30 - (i - 60)) * wstep; y = h; }
    else { x = 0.0f; y = (float)(30 - (i - 90)) * hstep; }
    return float2{x + margin, y + margin};
}
// interpolate_points(&[p0, p1, p2], 30)[i], i < 63 (:180-188)
__device__ __forceinline__ float2 gfw_zoom_interpolated(float2 p0, float2 p1, float2 p2, int i) {
    const int idx1 = i / 31;
    const float f = (float)(i % 31) / 31.0f;
    const float2 a = idx1 == 0 ? p0 : idx1 == 1 ? p1 : p2;
    const float2 b = idx1 == 0 ? p1 : p2;                                       // (idx1 + 1).min(len - 1)
    return float2{a.x + f * (b.x - a.x), a.y + f * (b.y - a.y)};
}
// nearest_edge (:136-151): the fold over the polygon in index order, from `m` on; -> the index accepted last, -1 = None
__device__ inline int gfw_zoom_nearest_edge(const float2 *poly, int n, float cx, float cy, float inv_aspect, float &m0, float &m1) {
    int idx = -1;
    for (int i = 0; i < n; ++i) {
        const float2 p = poly[i];
        const float ap0 = fabsf(p.x - cx), ap1 = fabsf(p.y - cy);
        if (ap0 < m0 && ap1 < m1) {
            if (ap1 > ap0 * inv_aspect) { m0 = ap1 / inv_aspect; m1 = ap1; }
            else { m0 = ap0; m1 = ap0 * inv_aspect; }
            idx = i;
        }
    }
    return idx;
}
// find_fov from the first undistort on (:95-133), by the lanes t = 0 .. GFW_ZOOM_LANES - 1 of a workgroup; `map(pass, i, x, y)` is undistort_points_with_rolling_shutter of one
// point followed by the centre offset (:99-102) — pass 0 the outline, pass k the k-th refinement.  -> nearest.1.0 (lane 0's value is the result).
// The loop `for _ in 1..5` as written, not as intended:
//   * `rect[idx]` — idx indexes the polygon folded last, which from the second round on is the 63-point refined one, yet picks among the 120 outline points;
//   * `rect[idx.overflowing_sub(1).0 % len]` — for idx = 0 that is usize::MAX % 120 = 15 (on 64- and 32-bit targets alike), not 119;
//   * a round whose second fold accepts nothing leaves nearest.0 = None only after the NEXT round has folded the same 63 points once more (from the current
//     rectangle: it accepts nothing new unless the f32 rounding of the first acceptance lets a point in) and then breaks.
template <typename Map>
__device__ __forceinline__ float gfw_zoom_rounds(const Map &map, int t, float w, float h, float margin, float inv_aspect, float2 *s_poly, int *s_idx, double *debug) {
    const float cx = w / 2.0f, cy = h / 2.0f;
    static_assert(GFW_ZOOM_LANES >= GFW_ZOOM_REFINED, "a refinement is one pass of the workgroup");
    for (int i = t; i < GFW_ZOOM_RECT; i += GFW_ZOOM_LANES) {                                       // two points per lane
        const float2 p = gfw_zoom_rect_point(i, w, h, margin);
        const float2 o = map(0, i, p.x, p.y);
        s_poly[i] = o;
        if (debug) { debug[i * 2] = (double)(o.x / w); debug[i * 2 + 1] = (double)(o.y / h); }      // :103-105
    }
    __syncthreads();
    int n_poly = GFW_ZOOM_RECT;
    float m0 = 1000000.0f, m1 = 1000000.0f * inv_aspect;                                           // lane 0's: nearest.1
    for (int round = 1; round < 5; ++round) {
        if (t == 0) *s_idx = gfw_zoom_nearest_edge(s_poly, n_poly, cx, cy, inv_aspect, m0, m1);
        __syncthreads();
        const int idx = *s_idx;
        if (idx < 0) break;                                                                          // workgroup-uniform
        float2 o = float2{0.0f, 0.0f};
        if (t < GFW_ZOOM_REFINED) {
            const float2 p0 = gfw_zoom_rect_point(idx == 0 ? 15 : idx - 1, w, h, margin);
            const float2 p1 = gfw_zoom_rect_point(idx, w, h, margin);
            const float2 p2 = gfw_zoom_rect_point((idx + 1) % GFW_ZOOM_RECT, w, h, margin);
            const float2 p = gfw_zoom_interpolated(p0, p1, p2, t);
            o = map(round, t, p.x, p.y);
        }
        if (t < GFW_ZOOM_REFINED) s_poly[t] = o;              // (lane 0 finished its fold of the old polygon before the barrier above)
        n_poly = GFW_ZOOM_REFINED;
        __syncthreads();
        if (t == 0) (void)gfw_zoom_nearest_edge(s_poly, n_poly, cx, cy, inv_aspect, m0, m1);       // its Option is overwritten by the next round's fold
    }
    return m0;
}

// at_timestamp_for_points' shift of one point (frame_transform.rs:412-429) in the 6-float form gfw_point_map takes (sx, sy, cos, sin, ox, oy).  `y`: the point's own y as
// given (0 for the single point of a frame without rolling shutter), under horizontal readout too.  Neither the framebuffer sign nor the sensor-height flip of the matrix
// path (frame_transform.rs:270-289) exists here; cos / sin of +angle, the host libm's (cpu_undistort.rs:753-755)
__device__ inline void gfw_zoom_shift(const GfwStab &S, double y, float out[6]) {
    const double y_sensor = (y - 0.0) * ((S.crop_y + S.crop_h) - S.crop_y) / (S.height - 0.0) + S.crop_y;            // map_coord, util.rs:144-147
    double sv[3], ov[3];
    if (!catmull_rom_at(S.ibis, S.ibis_n, y_sensor + S.offset, sv)) { sv[0] = 0.0; sv[1] = 0.0; sv[2] = 0.0; }        // unwrap_or_default()
    if (!catmull_rom_at(S.ois, S.ois_n, y_sensor + S.offset, ov)) { ov[0] = 0.0; ov[1] = 0.0; ov[2] = 0.0; }
    const float ra = (float)((sv[2] / 1000.0) * (3.14159265358979323846 / 180.0));                                  // to_radians() as f32
    out[0] = (float)(sv[0] * S.scale_x); out[1] = (float)(sv[1] * S.scale_y);
    out[2] = gfw_cosf(ra); out[3] = gfw_sinf(ra);
    out[4] = (float)(ov[0] * S.scale_x); out[5] = (float)(ov[1] * S.scale_y);
}

// STAB: the kernels of gfw_zoom_fovs_stab (gfw_zoom_stab_kernel) — per-point shifts from the frame's stabiliser splines and the frame's lens mesh
template <int MODEL, int STAB = 0>
struct GfwZoomMap {
    const gfw_kernel_params &P; const GfwCommon &C; const GfwTracks &T; const gfw_zoom_frame &F;
    const float *s_rot;              // LDS: the frame's one rotation (no rolling shutter, or given by the caller)
    Q pre;                           // smoothed(ts) * org(ts)^-1
    bool rolling, horizontal;
    double start_ts, row_readout_time;
    float amount, fov, cz0, cz1;
    const GfwStab *S;                // STAB: the frame's stabiliser data, or nullptr: no shifts (no entry; suppress_rotation = 2, frame_transform.rs:433-435)
    const double *mesh; int mesh_len;  // STAB: the frame's mesh
    __device__ __forceinline__ float2 operator()(int, int i, float x, float y) const {
        float rot[9];
        if (rolling) gfw_zoom_rotation(T, F, pre, start_ts + row_readout_time * (double)(horizontal ? x : y), rot);      // :393-394: the point as given, before the stretches
        else { for (int k = 0; k < 9; ++k) rot[k] = s_rot[k]; }
        float2 o;
        if constexpr (STAB) {
            // without rolling shutter points_iter is the single point (0, 0) (:389): ONE shift, which shift_per_point.get(index) hands to index 0 of each mapped set only
            float sh[6];
            const bool shifted = S && (rolling || i == 0);
            if (shifted) gfw_zoom_shift(*S, rolling ? (double)y : 0.0, sh);
            o = gfw_point_map<MODEL>(P, C, x, y, rot, shifted ? sh : nullptr, mesh, mesh_len, amount, fov);
        } else {
            o = gfw_point_map<MODEL>(P, C, x, y, rot, nullptr, nullptr, 0, amount, fov);
        }
        o.x -= cz0; o.y -= cz1;                                                                                          // fov_iterative.rs:99-102
        return o;
    }
};

// One wave per frame, two outline points per lane, rather than two waves with a point per lane: measured (tools/zoom_bench.py on the 10 000-frame clip,
// profiles/zoom_search.txt) 0.31 ms against 0.40 ms on the stream, 0.44-0.47 against 0.53-0.64 with lens_correction_amount 0.6 — a second wave idles through every
// refinement, and a one-wave workgroup leaves room for twice as many frames per CU.
template <int MODEL, int STAB>
__device__ __forceinline__ void gfw_zoom_frame_search(const gfw_kernel_params &P, const GfwCommon &C, const GfwZoomArgs &A) {
    __shared__ float2 s_poly[GFW_ZOOM_RECT];
    __shared__ float s_rot[9];
    __shared__ double s_pre[4];
    __shared__ int s_idx;
    const int t = threadIdx.x;
    const int f = blockIdx.x;
    const gfw_zoom_frame &F = A.frames[f];
    const double frt = F.frame_readout_time_ms;
    const bool rolling = fabs(frt) > 0.0;
    const double ts = F.timestamp_ms + F.per_frame_time_offset_ms;                  // frame_transform.rs:385-386
    const double start_ts = ts - frt / 2.0;
    const GfwStab *S = nullptr; const double *mesh = nullptr; int mesh_len = 0;
    if constexpr (STAB) {
        if (A.stabs && A.stabs[f].ibis_n >= 0 && F.suppress_rotation != 2) S = A.stabs + f;
        if (A.mesh_ref) { mesh = A.mesh_data + A.mesh_ref[f * 2]; mesh_len = A.mesh_ref[f * 2 + 1]; }
#if GFW_ZOOM_MESH_LDS
        __shared__ double s_mesh[GFW_ZOOM_MESH_MAX];                                // the frame's mesh, staged once: every point reads 72 of its entries at its own cell
        for (int k = t; k < mesh_len; k += GFW_ZOOM_LANES) s_mesh[k] = mesh[k];
        mesh = s_mesh;                                                              // (the barrier below orders it)
#endif
    }
    if (t == 0) {                                                                   // once per frame, not per point
        Q pre{1.0, 0.0, 0.0, 0.0};
        if (A.rotations) { for (int k = 0; k < 9; ++k) s_rot[k] = A.rotations[(size_t)f * 9 + k]; }
        else {
            if (!F.suppress_rotation) pre = quat_prefix(A.T, ts);
            if (!rolling) gfw_zoom_rotation(A.T, F, pre, start_ts, s_rot);
        }
        s_pre[0] = pre.w; s_pre[1] = pre.x; s_pre[2] = pre.y; s_pre[3] = pre.z;
    }
    __syncthreads();
    const GfwZoomMap<MODEL, STAB> map{P, C, A.T, F, s_rot, Q{s_pre[0], s_pre[1], s_pre[2], s_pre[3]}, rolling, A.horizontal != 0, start_ts,
                                      frt / (double)A.readout_dim, (float)F.lens_correction_amount, (float)F.fov,
                                      (float)F.zoom_center[0] * A.w, (float)F.zoom_center[1] * A.h, S, mesh, mesh_len};
    const float m0 = gfw_zoom_rounds(map, t, A.w, A.h, A.margin, A.inv_aspect, s_poly, &s_idx,
                                     A.debug_points ? A.debug_points + (size_t)f * (GFW_ZOOM_RECT * 2) : nullptr);
    if (t == 0) A.fov_minimal[f] = (double)(m0 * 2.0f / A.out_dim0);                // :133
}
template <int MODEL>
__global__ __launch_bounds__(GFW_ZOOM_LANES) void gfw_zoom_kernel(const gfw_kernel_params P, const GfwCommon C, const GfwZoomArgs A) {
    gfw_zoom_frame_search<MODEL, 0>(P, C, A);
}
// The instantiations of gfw_zoom_fovs_stab.  The f64 bivariate spline of the mesh (nine-entry coefficient arrays per axis) would take the wave past 256 registers, one
// wave per SIMD; two waves are asked for — a frame is one wave, and waves of other frames hide each other's spline and slerp latency.
template <int MODEL>
__global__ __launch_bounds__(GFW_ZOOM_LANES, 2) void gfw_zoom_stab_kernel(const gfw_kernel_params P, const GfwCommon C, const GfwZoomArgs A) {
    gfw_zoom_frame_search<MODEL, 1>(P, C, A);
}

hipError_t gfw_launch_zoom(const gfw_kernel_params &P, const GfwCommon &C, const GfwZoomArgs &A, int n_frames, hipStream_t s) {
    if (n_frames <= 0) return hipSuccess;
    const bool fisheye = C.model == GFW_MODEL_OPENCV_FISHEYE;
    if (A.stabs || A.mesh_ref) {
        if (fisheye) hipLaunchKernelGGL(gfw_zoom_stab_kernel<GFW_MODEL_OPENCV_FISHEYE>, dim3((unsigned)n_frames), dim3(GFW_ZOOM_LANES), 0, s, P, C, A);
        else hipLaunchKernelGGL(gfw_zoom_stab_kernel<-1>, dim3((unsigned)n_frames), dim3(GFW_ZOOM_LANES), 0, s, P, C, A);
    }
    else if (fisheye) hipLaunchKernelGGL(gfw_zoom_kernel<GFW_MODEL_OPENCV_FISHEYE>, dim3((unsigned)n_frames), dim3(GFW_ZOOM_LANES), 0, s, P, C, A);
    else hipLaunchKernelGGL(gfw_zoom_kernel<-1>, dim3((unsigned)n_frames), dim3(GFW_ZOOM_LANES), 0, s, P, C, A);
    return hipGetLastError();
}
