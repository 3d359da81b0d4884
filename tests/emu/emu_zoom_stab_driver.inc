// emu_zoom_stab_driver.inc — TEST INFRASTRUCTURE: launches of the zoom search's stabiliser / mesh kernels gfw_zoom_stab_kernel<MODEL> (gfw_zoom.hip, compiled for
// the host above) on the fibers, beside everything emu_zoom_driver.inc drives.  The host side is gfw_zoom_fovs_stab's own (gfw_zoom_host.h): the frames' GfwStab table
// with at_timestamp_for_points' scale, and the distinct meshes back to back with one (first value, length) pair per frame.
#include "emu_zoom_driver.inc"

static void emu_zoom_stab_body() {
    if (emu_cur->tid.y >= 1) return;
    if (emu_zC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_zoom_stab_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_zP, emu_zC, emu_zA);
    else gfw_zoom_stab_kernel<-1>(emu_zP, emu_zC, emu_zA);
}

// the arguments of gfw_emu_zoom, then gfw_zoom_fovs_stab's: stabs = [n_frames] gfw_frame_stab pointers or nullptr, meshes / mesh_lens = [n_frames] or nullptr
extern "C" int gfw_emu_zoom_stab(const void *kp, const void *common, const int64_t *org_ts, const double *org_q, int org_n, const int64_t *sm_ts, const double *sm_q, int sm_n,
                                 const int64_t *off_ts, const double *off_ms, int off_n, double duration_ms, const gfw_zoom_search *search,
                                 const gfw_zoom_frame *frames, int n_frames, const float *rotations, double *fov_minimal, double *debug_points,
                                 const gfw_frame_stab *const *stabs, const double *const *meshes, const size_t *mesh_lens) {
    emu_zoom_stage(kp, common, GfwTracks{org_ts, org_q, org_n, sm_ts, sm_q, sm_n, off_ts, off_ms, off_n, duration_ms}, search, frames, n_frames, rotations,
                   stabs, meshes, mesh_lens, fov_minimal, debug_points);
    if (!stabs && !meshes) return emu::run_grid(n_frames, emu_zoom_body);         // gfw_launch_zoom: no table, the plain instantiations
    return emu::run_grid(n_frames, emu_zoom_stab_body);
}
