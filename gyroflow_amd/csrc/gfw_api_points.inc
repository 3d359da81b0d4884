// gfw_api_points.inc — part of gfw_api.hip (textually included): the coordinate exports — gfw_undistort_points and the STMap map.  Their INPUTS are not staged through
// a ring like the other rows': they are millions of points (a map's pixels), the pageable copy was measured at the link's rate, and a pinned copy of them would cost
// what the ring saves.  Only the prologue and the outputs are the rows' common ones.

// Inverse point map (`undistort_points`, cpu_undistort.rs:652-858; the STMap "dist"
// pass stmap.rs:123-127 runs it per pixel).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_undistort_points(gfw_ctx *c, const gfw_kernel_params *p, const float *points, size_t n, int grid_width,
                                    const float *rotations, int rotation_count, const float *shifts, int index_mode,
                                    const double *mesh, size_t mesh_len, float *out, int out_on_device) {
    if (!c || !p || !rotations || !out || rotation_count < 1 || index_mode < 0 || index_mode > 3) { set_error("bad undistort_points arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!points && grid_width < 1) { set_error("grid_width must be >= 1 when points is NULL"); return GFW_ERR_INVALID_ARGUMENT; }
    if (mesh_len > GFW_MESH_MAX) { set_error("mesh too large"); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    API_TRY(validate_mesh(mesh, mesh_len));
    if (n == 0) return GFW_OK;                                               // :637 `if distorted.is_empty() { return Vec::new(); }`
    API_TRY(enter_device(c));
    GfwPointsArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.grid_w = grid_width; A.rotation_count = rotation_count; A.index_mode = index_mode;
    const size_t pts_bytes = n * 2 * sizeof(float);
    if (points) {
        HIP_TRY(c->d_pts_in.ensure(pts_bytes), GFW_ERR_HIP);
        HIP_TRY(hipMemcpyAsync(c->d_pts_in.ptr, points, pts_bytes, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
        A.points = (const float *)c->d_pts_in.ptr;
    }
    HIP_TRY(c->d_pts_rot.ensure((size_t)rotation_count * 9 * sizeof(float)), GFW_ERR_HIP);
    HIP_TRY(hipMemcpyAsync(c->d_pts_rot.ptr, rotations, (size_t)rotation_count * 9 * sizeof(float), hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    A.rotations = (const float *)c->d_pts_rot.ptr;
    std::vector<float> packed;
    if (shifts) {
        // cos/sin of the roll angle by the host libm, exactly what the reference evaluates per point (:756-757)
        packed.resize((size_t)rotation_count * 6);
        for (int i = 0; i < rotation_count; ++i) {
            const float *s = shifts + (size_t)i * 5;
            float *d = packed.data() + (size_t)i * 6;
            d[0] = s[0]; d[1] = s[1]; d[2] = cosf(s[2]); d[3] = sinf(s[2]); d[4] = s[3]; d[5] = s[4];
        }
        HIP_TRY(c->d_pts_shift.ensure(packed.size() * sizeof(float)), GFW_ERR_HIP);
        HIP_TRY(hipMemcpyAsync(c->d_pts_shift.ptr, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
        A.shifts = (const float *)c->d_pts_shift.ptr;
    }
    if (mesh && mesh_len) {
        HIP_TRY(c->d_pts_mesh.ensure(mesh_len * sizeof(double)), GFW_ERR_HIP);
        HIP_TRY(hipMemcpyAsync(c->d_pts_mesh.ptr, mesh, mesh_len * sizeof(double), hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
        A.mesh = (const double *)c->d_pts_mesh.ptr; A.mesh_len = (int)mesh_len;
    }
    CallOutputs O(c->d_out, out_on_device);
    O.add(out, pts_bytes);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    A.out = (float *)O.dev(0);
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    HIP_TRY(gfw_launch_points(*p, C, A, c->stream), GFW_ERR_HIP);
    c->last_backend = "points";
    // host staging vectors (packed shifts) and pageable copies: always complete before returning
    HIP_TRY(O.finish(c->stream, true), GFW_ERR_HIP);
    return GFW_OK;
}

// STMap "undist" coordinate map (src/core/stmap.rs:87-109, :127-137): coords is width*height*2 f32, host or device
// memory (coords_on_device); pixels whose projection is None keep their previous content, as parallel_exr leaves 0.
extern "C" int gfw_stmap_undistort(gfw_ctx *c, const gfw_kernel_params *p, const float *matrices, int matrix_count,
                                   const float *mesh, size_t mesh_len, int width, int height, float *coords, int coords_on_device) {
    if (!c || !p || !coords || width < 1 || height < 1) { set_error("bad stmap arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    if (p->matrix_count != matrix_count || matrix_count < 1) { set_error("matrix_count %d != %d", p->matrix_count, matrix_count); return GFW_ERR_INVALID_ARGUMENT; }
    if (mesh_len > GFW_MESH_MAX) { set_error("mesh too large"); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    API_TRY(validate_mesh(mesh, mesh_len));
    API_TRY(enter_device(c));
    const float *d_mat = nullptr;
    API_TRY(upload_matrices(c, matrices, matrix_count, &d_mat));
    const float *d_mesh = nullptr;
    if (mesh && mesh_len) { HIP_TRY(hipMemcpyAsync(c->d_mesh.ptr, mesh, mesh_len * sizeof(float), hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP); d_mesh = (const float *)c->d_mesh.ptr; }
    GfwCommon C;
    fill_common(c, p, d_mat, d_mesh, (int)mesh_len, C);
    const size_t bytes = (size_t)width * height * 2 * sizeof(float);
    CallOutputs O(c->d_out, coords_on_device);
    O.add(coords, bytes);
    HIP_TRY(O.reserve(), GFW_ERR_HIP);
    float *d_coords = (float *)O.dev(0);
    // (the map goes up first: a pixel whose ray is rejected keeps what the caller's map held)
    if (!coords_on_device) HIP_TRY(hipMemcpyAsync(d_coords, coords, bytes, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_stmap(*p, C, width, height, d_coords, c->stream), GFW_ERR_HIP);
    c->last_backend = "stmap";
    API_TRY(matrices_consumed(c));
    HIP_TRY(O.finish(c->stream, c->synchronous), GFW_ERR_HIP);
    return GFW_OK;
}
