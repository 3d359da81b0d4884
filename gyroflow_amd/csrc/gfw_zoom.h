// gfw_zoom.h — the adaptive-zoom FOV search on the device (gfw_zoom.hip): FovIterative::find_fov for every frame of a clip
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_matrices.h"

#define GFW_ZOOM_RECT 120           // points_around_rect(w, h, 31, 31): (30 + 30) * 2
#define GFW_ZOOM_REFINED 63         // interpolate_points(3 points, 30): 31 * 3 - 30
#define GFW_ZOOM_LANES 64           // lanes of a frame's workgroup: one wave, two outline points per lane

struct GfwZoomArgs {
    GfwTracks T;                    // the context's tracks (read only when rotations == nullptr)
    const gfw_zoom_frame *frames;   // [n_frames] (device)
    const float *rotations;         // [n_frames][9] f32 (device) or nullptr
    double *fov_minimal;            // [n_frames] (device)
    double *debug_points;           // [n_frames][120][2] (device) or nullptr
    int32_t horizontal;             // the point's x picks its time
    float w, h;                     // input_dim
    float margin;                   // fov_algorithm_margin
    float out_dim0;                 // output_dim.0 = org_output_width as f32 * (width as f32 / org_output_width.max(1) as f32)
    float inv_aspect;               // output_dim.1 / output_dim.0
    int32_t readout_dim;            // width (horizontal readout) or height
    // gfw_zoom_fovs_stab (appended; all zero = none: the plain instantiations are launched)
    const GfwStab *stabs;           // [n_frames] (device) or nullptr: camera_stab_data[frame]; ibis_n < 0 = no entry for the frame.  scale_x / scale_y are
                                    // at_timestamp_for_points' is_scale (no framebuffer sign), sensor_h is not read
    const double *mesh_data;        // the clip's distinct f64 meshes back to back (device) or nullptr
    const int32_t *mesh_ref;        // [n_frames][2] (device) or nullptr: the frame's mesh as (first double in mesh_data, length; 0 = none)
};
#define GFW_ZOOM_MESH_MAX 839       // MAX_BUFFER_SIZE (gyro_source/splines.rs:88-89): the longest mesh a frame can name
// `n_frames` frames in one launch, one workgroup each
hipError_t gfw_launch_zoom(const gfw_kernel_params &P, const GfwCommon &C, const GfwZoomArgs &A, int n_frames, hipStream_t s);
