// emu_zoom_stab_driver.inc — TEST INFRASTRUCTURE: launches of the zoom search's stabiliser / mesh kernels gfw_zoom_stab_kernel<MODEL> (gfw_zoom.hip, compiled for
// the host above) on the fibers, beside everything emu_zoom_driver.inc drives.  The host side (tests/_zoomstab.py) restates what gfw_zoom_fovs_stab prepares: the frames'
// GfwStab table with at_timestamp_for_points' scale, and the meshes back to back with one (first value, length) pair per frame.
#include "emu_zoom_driver.inc"

static void emu_zoom_stab_body() {
    if (emu_cur->tid.y >= 1) return;
    if (emu_zC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_zoom_stab_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_zP, emu_zC, emu_zA);
    else gfw_zoom_stab_kernel<-1>(emu_zP, emu_zC, emu_zA);
}

// the arguments of gfw_emu_zoom, then: stabs = [n_frames] GfwStab or nullptr, mesh_data / mesh_ref = GfwZoomArgs' or nullptr
extern "C" int gfw_emu_zoom_stab(const void *kp, const void *common, const int64_t *org_ts, const double *org_q, int org_n, const int64_t *sm_ts, const double *sm_q, int sm_n,
                                 const int64_t *off_ts, const double *off_ms, int off_n, double duration_ms, const int *search, float margin,
                                 const void *frames, int n_frames, const float *rotations, double *fov_minimal, double *debug_points,
                                 const void *stabs, const double *mesh_data, const int32_t *mesh_ref) {
    // a launch of no workgroup: fills the argument block as gfw_emu_zoom does
    const int rc = gfw_emu_zoom(kp, common, org_ts, org_q, org_n, sm_ts, sm_q, sm_n, off_ts, off_ms, off_n, duration_ms, search, margin, frames, 0, rotations, fov_minimal, debug_points);
    if (rc) return rc;
    emu_zA.stabs = static_cast<const GfwStab *>(stabs); emu_zA.mesh_data = mesh_data; emu_zA.mesh_ref = mesh_ref;
    if (!stabs && !mesh_ref) return emu::run_grid(n_frames, emu_zoom_body);       // gfw_launch_zoom: no table, the plain instantiations
    return emu::run_grid(n_frames, emu_zoom_stab_body);
}
