// gfw_matrices.hip — per-row rolling-shutter matrices built on the device.
//
// The step immediately before the warp kernel: FrameTransform::at_timestamp (src/core/stabilization/
// frame_transform.rs:221-308) evaluates, for every sensor row y,
//     quat  = smoothed(ts) * org(ts)^-1 * org(start_ts + row_readout_time * y)
//     R     = image_rotation * R(quat), with the framebuffer sign flips (:261-267)
//     row_y = f32( inv(new_k * R) )
// on the host with rayon + an f64 SVD pseudo-inverse and uploads 14 floats per row every frame.  Here one lane
// does one row in f64 — quaternion lookup with the reference's rounding/clamping and nalgebra's slerp
// (src/core/gyro_source/mod.rs:857-882), closed-form 3x3 inverse — and writes libgfwarp's packed 64-byte row straight
// into HBM, so the per-frame host->device traffic of this path drops from 121 KB to a 160-byte descriptor.
// Parity is tolerance-based by construction (SVD vs adjugate inverse, ocml vs libm acos/sin): tests compare the rows
// with the float64 host statement to <= 2 ULP of f32 and then warp with the device-built rows bit-exactly.
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_matrices.h"
#include "gfw_math.h"
#include "gfw_quat.h"
#include "gfw_spline.h"

namespace {

// The row-independent factor smoothed(ts) * org(ts)^-1 (frame_transform.rs:255-256,289-291), once per frame: a
// one-lane kernel in front of the row kernel, so that the 34 row waves do one slerp each instead of three.
// Batched form: `frames` frame descriptors in device memory, one prefix lane per frame, blockIdx.y = frame.
__global__ void gfw_build_prefix_kernel(const GfwTracks T, const gfw_frame_timing *Fs, int frames, double *prefix) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= frames) return;
    const gfw_frame_timing &F = Fs[f];
    prefix += (size_t)f * 4;
    const double ts = F.timestamp_ms + F.per_frame_time_offset_ms;
    const Q pre = quat_prefix(T, ts);
    prefix[0] = pre.w; prefix[1] = pre.x; prefix[2] = pre.y; prefix[3] = pre.z;
}
// One row of one frame's table (frame_transform.rs:249-308): the body of both row kernels below — `S` by value for a whole launch, or the frame's entry of a device table
__device__ __forceinline__ void gfw_build_matrices_row(const GfwTracks &T, const gfw_frame_timing &F, const double *prefix, float *out, const GfwStab &S) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= F.rows) return;
    const double frt = F.frame_readout_time_ms;
    const double ts = F.timestamp_ms + F.per_frame_time_offset_ms;
    const double start_ts = ts - frt / 2.0;
    const double row_t = frt / (double)F.readout_dim;
    const double qt = (fabs(frt) > 0.0) ? start_ts + row_t * (double)y : start_ts;
    const Q pre{prefix[0], prefix[1], prefix[2], prefix[3]};
    Q q = qmul(pre, quat_at(T, T.org_ts, T.org_q, T.org_n, qt));
    double r[3][3];
    quat_rotation(q, F.video_rotation_deg, r);
    if (F.framebuffer_inverted) { r[0][2] *= -1.0; r[1][2] *= -1.0; r[2][0] *= -1.0; r[2][1] *= -1.0; }
    else { r[0][1] *= -1.0; r[0][2] *= -1.0; r[1][0] *= -1.0; r[2][0] *= -1.0; }
    // IBIS / OIS terms of this row (frame_transform.rs:270-289)
    float sx = 0.0f, sy = 0.0f, ra = 0.0f, ox = 0.0f, oy = 0.0f;
    if (S.ibis_n >= 0) {
        double y_sensor = ((double)y - 0.0) * ((S.crop_y + S.crop_h) - S.crop_y) / (S.height - 0.0) + S.crop_y;      // map_coord, util.rs:144-147
        if (F.framebuffer_inverted) y_sensor = S.sensor_h - y_sensor;
        double sv[3] = {0.0, 0.0, 0.0}, ov[3] = {0.0, 0.0, 0.0};
        if (!catmull_rom_at(S.ibis, S.ibis_n, y_sensor + S.offset, sv)) { sv[0] = 0.0; sv[1] = 0.0; sv[2] = 0.0; }
        if (!catmull_rom_at(S.ois, S.ois_n, y_sensor + S.offset, ov)) { ov[0] = 0.0; ov[1] = 0.0; ov[2] = 0.0; }
        const double rad = sv[2] / 1000.0 * (F.framebuffer_inverted ? -1.0 : 1.0);
        sx = (float)(sv[0] * S.scale_x); sy = (float)(sv[1] * S.scale_y);
        ra = (float)(rad * (3.14159265358979323846 / 180.0));      // to_radians()
        ox = (float)(ov[0] * S.scale_x); oy = (float)(ov[1] * S.scale_y);
    }
    if (F.suppress_rotation) {                                     // :291-296
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r[i][j] = (i == j) ? 1.0 : 0.0;
        if (F.suppress_rotation == 2) { sx = 0.0f; sy = 0.0f; ra = 0.0f; ox = 0.0f; oy = 0.0f; }
    }
    double m[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m[i][j] = F.new_k[i * 3 + 0] * r[0][j] + F.new_k[i * 3 + 1] * r[1][j] + F.new_k[i * 3 + 2] * r[2][j];
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    const double id = 1.0 / det;
    float *o = out + (size_t)y * GFW_MAT_STRIDE;
    o[0] = (float)(c00 * id); o[1] = (float)((m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id); o[2] = (float)((m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id);
    o[3] = (float)(c01 * id); o[4] = (float)((m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id); o[5] = (float)((m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id);
    o[6] = (float)(c02 * id); o[7] = (float)((m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id); o[8] = (float)((m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id);
    o[9] = sx; o[10] = sy; o[11] = ra; o[12] = ox; o[13] = oy;
    // cos/sin of the roll as cpu_undistort.rs:159-160 evaluates them (host libm, restated in gfw_math.h), only for rows with data
    if (sx != 0.0f || sy != 0.0f || ra != 0.0f || ox != 0.0f || oy != 0.0f) { o[14] = gfw_cosf(-ra); o[15] = gfw_sinf(-ra); }
    else { o[14] = 1.0f; o[15] = 0.0f; }
}
__global__ void gfw_build_matrices_kernel(const GfwTracks T, const gfw_frame_timing *Fs, const double *prefix, float *out, size_t table_floats, const GfwStab S) {
    gfw_build_matrices_row(T, Fs[blockIdx.y], prefix + (size_t)blockIdx.y * 4, out + (size_t)blockIdx.y * table_floats, S);
}
// The same with every frame's own stabiliser data: `Ss[frames]` in device memory (counts of -1: the frame has none), blockIdx.y = frame
__global__ void gfw_build_matrices_stab_kernel(const GfwTracks T, const gfw_frame_timing *Fs, const double *prefix, float *out, size_t table_floats, const GfwStab *Ss) {
    gfw_build_matrices_row(T, Fs[blockIdx.y], prefix + (size_t)blockIdx.y * 4, out + (size_t)blockIdx.y * table_floats, Ss[blockIdx.y]);
}

}  // namespace

hipError_t gfw_launch_build_matrices(const GfwTracks &T, const gfw_frame_timing *d_timings, int frames, int max_rows, double *prefix_scratch,
                                     float *out, size_t table_floats, hipStream_t s, const GfwStab *stab) {
    if (frames <= 0 || max_rows <= 0) return hipSuccess;
    GfwStab S;
    if (stab) S = *stab; else { S = GfwStab{0, 0, 0, 0, 0, 0, 0, nullptr, nullptr, -1, -1}; }
    hipLaunchKernelGGL(gfw_build_prefix_kernel, dim3((frames + 63) / 64), dim3(64), 0, s, T, d_timings, frames, prefix_scratch);
    hipLaunchKernelGGL(gfw_build_matrices_kernel, dim3((max_rows + 63) / 64, frames), dim3(64), 0, s, T, d_timings, (const double *)prefix_scratch, out, table_floats, S);
    return hipGetLastError();
}
hipError_t gfw_launch_build_matrices_stab(const GfwTracks &T, const gfw_frame_timing *d_timings, int frames, int max_rows, double *prefix_scratch,
                                          float *out, size_t table_floats, hipStream_t s, const GfwStab *d_stabs) {
    if (frames <= 0 || max_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_build_prefix_kernel, dim3((frames + 63) / 64), dim3(64), 0, s, T, d_timings, frames, prefix_scratch);
    hipLaunchKernelGGL(gfw_build_matrices_stab_kernel, dim3((max_rows + 63) / 64, frames), dim3(64), 0, s, T, d_timings, (const double *)prefix_scratch, out, table_floats, d_stabs);
    return hipGetLastError();
}
