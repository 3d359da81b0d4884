// gfw_api_zoom.inc — part of gfw_api.hip (textually included): the adaptive zoom's entry points — gfw_zoom_fovs, gfw_zoom_fovs_stab, gfw_zoom_smooth.  What they
// stage and the host half's arithmetic are gfw_zoom_host.h's.

// Adaptive zoom, first half: FovIterative::find_fov of every frame (fov_iterative.rs:91-134) in one launch, a workgroup per frame (gfw_zoom.hip).
// See include/gfwarp.h for the argument contract.  `with_data`: gfw_zoom_fovs_stab — per-frame stabiliser data and meshes are taken, the three data flags are not
// consulted, suppress_rotation 2 is a value.
static int zoom_fovs_impl(gfw_ctx *c, const gfw_kernel_params *p, const gfw_zoom_search *search, const gfw_zoom_frame *frames, int n_frames, const float *rotations,
                          const gfw_frame_stab *const *stabs, const double *const *meshes, const size_t *mesh_lens,
                          double *fov_minimal, double *debug_points, int out_on_device, bool with_data) {
    if (!c || !p || !search || n_frames < 0) { set_error("bad zoom arguments (null context / params / search, or n_frames < 0)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_frames == 0) return GFW_OK;                                        // fov_iterative.rs:33 `if timestamps.is_empty() { return Vec::new(); }`
    if (!frames || !fov_minimal) { set_error("bad zoom arguments (null frames / fov_minimal)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (meshes && !mesh_lens) { set_error("bad zoom arguments (meshes without mesh_lens)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (search->width < 1 || search->height < 1 || search->org_output_width < 1 || search->org_output_height < 1 || !(search->fov_algorithm_margin == search->fov_algorithm_margin) ||
        search->horizontal_readout < 0 || search->horizontal_readout > 1) {
        set_error("bad zoom search: %d x %d, output %d x %d, margin %g, horizontal_readout %d", search->width, search->height, search->org_output_width, search->org_output_height,
                  (double)search->fov_algorithm_margin, search->horizontal_readout);
        return GFW_ERR_INVALID_ARGUMENT; }
    if (!with_data && (p->flags & (256 | 512 | 1024))) {                     // HAS_IBIS_DATA | HAS_MESH_DATA | HAS_FPD_DATA
        set_error("the zoom search does not cover per-frame IBIS/OIS shifts, lens meshes or focal-plane distortion data (flags 0x%x): map the outline with gfw_undistort_points", p->flags);
        return GFW_ERR_INVALID_ARGUMENT; }
    if (!rotations && c->tracks.org_n < 1 && c->tracks.sm_n < 1) { set_error("no rotations given and no quaternion tracks set (gfw_set_quaternion_tracks)"); return GFW_ERR_INVALID_ARGUMENT; }
    for (int i = 0; i < n_frames; ++i) {
        if (frames[i].suppress_rotation < 0 || frames[i].suppress_rotation > (with_data ? 2 : 1)) { set_error("frame %d: suppress_rotation %d", i, frames[i].suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
        if (rotations && frames[i].frame_readout_time_ms != 0.0) {
            set_error("frame %d: caller-given rotations are one per frame, but frame_readout_time_ms = %g needs one per point", i, frames[i].frame_readout_time_ms);
            return GFW_ERR_INVALID_ARGUMENT; }
        if (stabs && stabs[i] && !stab_ok(stabs[i], i)) return GFW_ERR_INVALID_ARGUMENT;
        if (meshes && mesh_lens[i]) {
            if (!meshes[i]) { set_error("frame %d: mesh of %zu values is NULL", i, mesh_lens[i]); return GFW_ERR_INVALID_ARGUMENT; }
            if (gfw_zoom_mesh_repeats(meshes, mesh_lens, i)) continue;                                    // the mesh of the frame before: checked and uploaded once
            if (mesh_lens[i] > GFW_MESH_MAX) { set_error("frame %d: mesh too large (%zu values, at most %d)", i, mesh_lens[i], GFW_MESH_MAX); return GFW_ERR_INVALID_ARGUMENT; }
            if (validate_mesh(meshes[i], mesh_lens[i]) != GFW_OK) { const std::string why = g_last_error; set_error("frame %d: %s", i, why.c_str()); return GFW_ERR_INVALID_ARGUMENT; }
        }
    }
    // the sizes of the block's two variable parts, by the packers' own count
    const size_t point_bytes = stabs ? gfw_stab_points_total(stabs, n_frames) : 0, mesh_doubles = meshes ? gfw_zoom_mesh_doubles(meshes, mesh_lens, n_frames) : 0;
    if (mesh_doubles > 0x7fffffffu) { set_error("the clip's distinct meshes hold %zu values: more than a frame's 32-bit mesh reference addresses", mesh_doubles); return GFW_ERR_INVALID_ARGUMENT; }
    static_assert(GFW_MESH_MAX == GFW_ZOOM_MESH_MAX, "one mesh limit");
    API_TRY(enter_device(c));
    // descriptors (rotations, stabiliser tables, control points, meshes) through pinned memory in one copy: it is enqueued, the caller's arrays are free on return.
    // The slot is free when the copy that last read the pinned block is done; a launch in flight that still reads a device block about to be replaced is waited for
    const GfwZoomLayout Z = gfw_zoom_layout(n_frames, rotations != nullptr, stabs != nullptr, point_bytes, meshes != nullptr, mesh_doubles);
    GfwZoomArgs A;
    memset(&A, 0, sizeof(A));
    StagedBlock B;
    HIP_TRY(c->zoom_ring.acquire(Z.total, c->stream, &B.slot), GFW_ERR_HIP);
    gfw_zoom_fill(Z, frames, n_frames, rotations, stabs, meshes, mesh_lens, B.h(), B.d(), A);
    HIP_TRY(B.upload(Z.total, c->stream), GFW_ERR_HIP);
    HIP_TRY(B.free_again(c->stream), GFW_ERR_HIP);
    CallOutputs O(c->d_out, out_on_device);
    O.add(fov_minimal, sizeof(double) * (size_t)n_frames);
    O.add(debug_points, sizeof(double) * 2 * GFW_ZOOM_RECT * (size_t)n_frames);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    A.T = c->tracks;
    A.fov_minimal = (double *)O.dev(0); A.debug_points = (double *)O.dev(1);
    gfw_zoom_search_args(*search, A);
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    HIP_TRY(gfw_launch_zoom(*p, C, A, n_frames, c->stream), GFW_ERR_HIP);
    c->last_backend = (stabs || meshes) ? "zoom_fovs_stab" : "zoom_fovs";
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    return GFW_OK;
}
extern "C" int gfw_zoom_fovs(gfw_ctx *c, const gfw_kernel_params *p, const gfw_zoom_search *search, const gfw_zoom_frame *frames, int n_frames,
                             const float *rotations, double *fov_minimal, double *debug_points, int out_on_device) {
    return zoom_fovs_impl(c, p, search, frames, n_frames, rotations, nullptr, nullptr, nullptr, fov_minimal, debug_points, out_on_device, false);
}
// The same for clips with camera_stab_data and a per-frame mesh_correction (frame_transform.rs:370-373, :412-435): NULL tables launch gfw_zoom_fovs's own instantiations.
extern "C" int gfw_zoom_fovs_stab(gfw_ctx *c, const gfw_kernel_params *p, const gfw_zoom_search *search, const gfw_zoom_frame *frames, int n_frames,
                                  const float *rotations, const gfw_frame_stab *const *stabs, const double *const *meshes, const size_t *mesh_lens,
                                  double *fov_minimal, double *debug_points, int out_on_device) {
    return zoom_fovs_impl(c, p, search, frames, n_frames, rotations, stabs, meshes, mesh_lens, fov_minimal, debug_points, out_on_device, true);
}

// Adaptive zoom, second half, on the host (gfw_zoom_smooth_host)
extern "C" int gfw_zoom_smooth(const double *fov_minimal, int n, double adaptive_zoom_window, double scaled_fps, int method,
                               const double *trim_ranges, int n_ranges, double *fovs_out, double *fov_minimal_out) {
    if (n < 0 || n_ranges < 0 || (n && (!fov_minimal || !fovs_out)) || (n_ranges && !trim_ranges) || !(adaptive_zoom_window == adaptive_zoom_window)) {
        set_error("bad zoom_smooth arguments (n %d, n_ranges %d, window %g)", n, n_ranges, adaptive_zoom_window); return GFW_ERR_INVALID_ARGUMENT; }
    if (adaptive_zoom_window > 0.0001 && !(scaled_fps > 0.0)) { set_error("scaled_fps %g", scaled_fps); return GFW_ERR_INVALID_ARGUMENT; }
    if (n) gfw_zoom_smooth_host(fov_minimal, n, adaptive_zoom_window, scaled_fps, method, trim_ranges, n_ranges, fovs_out, fov_minimal_out);
    return GFW_OK;
}
