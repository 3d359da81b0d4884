// gfw_api_adjacent.inc — part of gfw_api.hip (textually included): the entry points of the rows next to the warp (SURVEY.md section 8f) — the per-row matrix
// builder (gfw_set_quaternion_tracks, gfw_build_matrices*), gfw_undistort_points, the STMap export, the zoom search, the sync search.  Split out of gfw_api.hip in round 6.


extern "C" {
int gfw_set_quaternion_tracks(gfw_ctx *c, const int64_t *org_ts, const double *org_q, int org_n,
                              const int64_t *sm_ts, const double *sm_q, int sm_n) {
    if (!c || org_n < 0 || sm_n < 0 || (org_n && (!org_ts || !org_q)) || (sm_n && (!sm_ts || !sm_q))) { set_error("bad track arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    for (int i = 1; i < org_n; ++i) if (org_ts[i] <= org_ts[i - 1]) { set_error("original track timestamps must ascend"); return GFW_ERR_INVALID_ARGUMENT; }
    for (int i = 1; i < sm_n; ++i) if (sm_ts[i] <= sm_ts[i - 1]) { set_error("smoothed track timestamps must ascend"); return GFW_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    const size_t b0 = (size_t)org_n * 8, b1 = (size_t)org_n * 32, b2 = (size_t)sm_n * 8, b3 = (size_t)sm_n * 32;
    HIP_TRY(c->d_tracks.ensure(b0 + b1 + b2 + b3 + 64), GFW_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    char *base = (char *)c->d_tracks.ptr;
    if (org_n) { HIP_TRY(hipMemcpy(base, org_ts, b0, hipMemcpyHostToDevice), GFW_ERR_HIP); HIP_TRY(hipMemcpy(base + b0, org_q, b1, hipMemcpyHostToDevice), GFW_ERR_HIP); }
    if (sm_n) { HIP_TRY(hipMemcpy(base + b0 + b1, sm_ts, b2, hipMemcpyHostToDevice), GFW_ERR_HIP); HIP_TRY(hipMemcpy(base + b0 + b1 + b2, sm_q, b3, hipMemcpyHostToDevice), GFW_ERR_HIP); }
    c->tracks.org_ts = (const int64_t *)base; c->tracks.org_q = (const double *)(base + b0); c->tracks.org_n = org_n;
    c->tracks.sm_ts = (const int64_t *)(base + b0 + b1); c->tracks.sm_q = (const double *)(base + b0 + b1 + b2); c->tracks.sm_n = sm_n;
    return GFW_OK;
}
int gfw_set_sync_offsets(gfw_ctx *c, double duration_ms, const int64_t *ts_us, const double *offsets_ms, int count) {
    if (!c || count < 0 || (count && (!ts_us || !offsets_ms)) || !(duration_ms == duration_ms)) { set_error("bad sync-offset arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    for (int i = 1; i < count; ++i) if (ts_us[i] <= ts_us[i - 1]) { set_error("sync-offset timestamps must ascend"); return GFW_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream), GFW_ERR_HIP);
    c->tracks.duration_ms = duration_ms; c->tracks.off_n = count; c->tracks.off_ts = nullptr; c->tracks.off_ms = nullptr;
    if (count) {
        HIP_TRY(c->d_offsets.ensure((size_t)count * 16), GFW_ERR_HIP);
        char *base = (char *)c->d_offsets.ptr;
        HIP_TRY(hipMemcpy(base, ts_us, (size_t)count * 8, hipMemcpyHostToDevice), GFW_ERR_HIP);
        HIP_TRY(hipMemcpy(base + (size_t)count * 8, offsets_ms, (size_t)count * 8, hipMemcpyHostToDevice), GFW_ERR_HIP);
        c->tracks.off_ts = (const int64_t *)base; c->tracks.off_ms = (const double *)(base + (size_t)count * 8);
    }
    return GFW_OK;
}
// Copies `count` frame descriptors through the next slot of the timings ring on `stream`; the caller records the slot's free_again behind the builder it launches
// (the builder reads the device side, on whichever of the context's two streams this build runs: the slot is not free while it may)
static int stage_timings(gfw_ctx *c, const gfw_frame_timing *t, int count, hipStream_t stream, StagingSlot **out) {
    const size_t slot_bytes = sizeof(gfw_frame_timing) * gfw_ctx::kMaxBatch;
    if (!c->timing_ring.slots[0].d.ptr) HIP_TRY(c->timing_ring.reserve(slot_bytes), GFW_ERR_HIP);
    HIP_TRY(c->timing_ring.acquire(slot_bytes, stream, out), GFW_ERR_HIP);
    memcpy((*out)->h.ptr, t, sizeof(gfw_frame_timing) * count);
    HIP_TRY(hipMemcpyAsync((*out)->d.ptr, (*out)->h.ptr, sizeof(gfw_frame_timing) * count, hipMemcpyHostToDevice, stream), GFW_ERR_HIP);
    return GFW_OK;
}
static bool timing_ok(const gfw_frame_timing *t) { return t->rows >= 1 && t->readout_dim >= 1 && t->suppress_rotation >= 0 && t->suppress_rotation <= 2; }
// gfw_frame_stab as every entry that takes one checks it: counts >= 0 with their arrays, non-zero crop and pitch, ascending spline positions.  `frame` >= 0 is named in the error.
static bool stab_ok(const gfw_frame_stab *stab, int frame) {
    char who[32] = "";
    if (frame >= 0) snprintf(who, sizeof(who), "frame %d: ", frame);
    if (stab->ibis_count < 0 || stab->ois_count < 0 || (stab->ibis_count && !stab->ibis) || (stab->ois_count && !stab->ois) ||
        !(stab->crop_area[2] != 0.0) || !(stab->crop_area[3] != 0.0) || !(stab->pixel_pitch[0] != 0.0) || !(stab->pixel_pitch[1] != 0.0)) {
        set_error("%sbad stabiliser data (counts %d/%d, crop %g x %g, pitch %g x %g)", who, stab->ibis_count, stab->ois_count, stab->crop_area[2], stab->crop_area[3], stab->pixel_pitch[0], stab->pixel_pitch[1]);
        return false; }
    for (int i = 1; i < stab->ibis_count; ++i) if (!(stab->ibis[i * 4] >= stab->ibis[(i - 1) * 4])) { set_error("%sIBIS spline positions must ascend", who); return false; }
    for (int i = 1; i < stab->ois_count; ++i) if (!(stab->ois[i * 4] >= stab->ois[(i - 1) * 4])) { set_error("%sOIS spline positions must ascend", who); return false; }
    return true;
}
static size_t stab_point_bytes(const gfw_frame_stab *stab) { return ((size_t)stab->ibis_count + (size_t)stab->ois_count) * 32; }
// The device form of a frame's stabiliser data; its control points are copied to `h_points` (pinned), which the caller uploads to `d_points`.  y_sign: the
// framebuffer sign of the matrix path (frame_transform.rs:234-241), 1.0 for at_timestamp_for_points (:413-416)
static GfwStab stab_device(const gfw_frame_stab *stab, double y_sign, void *h_points, const void *d_points) {
    const size_t nb0 = (size_t)stab->ibis_count * 32, nb1 = (size_t)stab->ois_count * 32;
    if (nb0) memcpy(h_points, stab->ibis, nb0);
    if (nb1) memcpy((char *)h_points + nb0, stab->ois, nb1);
    GfwStab S;
    S.offset = stab->offset; S.sensor_h = stab->sensor_size[1]; S.crop_y = stab->crop_area[1]; S.crop_h = stab->crop_area[3];
    S.scale_x = stab->width / stab->crop_area[2] / stab->pixel_pitch[0];
    S.scale_y = stab->height / stab->crop_area[3] / stab->pixel_pitch[1] * y_sign;
    S.height = stab->height;
    S.ibis = (const double *)d_points; S.ois = (const double *)((const char *)d_points + nb0); S.ibis_n = stab->ibis_count; S.ois_n = stab->ois_count;
    return S;
}
static const GfwStab kNoStab = {0, 0, 0, 0, 0, 0, 0, nullptr, nullptr, -1, -1};

int gfw_build_matrices(gfw_ctx *c, const gfw_frame_timing *t, float *rows16_out, float **out_ptr) {
    return gfw_build_matrices_stab(c, t, nullptr, rows16_out, out_ptr);
}
int gfw_build_matrices_stab(gfw_ctx *c, const gfw_frame_timing *t, const gfw_frame_stab *stab, float *rows16_out, float **out_ptr) {
    if (!c || !t) { set_error("null context/timing"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!timing_ok(t)) { set_error("rows %d, readout_dim %d, suppress_rotation %d", t->rows, t->readout_dim, t->suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    // a caller-owned table is built in order on the context's stream; a context-owned one in the next slot of the ring, on the auxiliary stream (overlaps the warp in flight)
    const hipStream_t stream = rows16_out ? c->stream : c->copy_stream;
    GfwStab S, *Sp = nullptr;
    StagingSlot *stab_slot = nullptr, *t_slot = nullptr; size_t stab_bytes = 0;
    if (stab) {
        if (!stab_ok(stab, -1)) return GFW_ERR_INVALID_ARGUMENT;
        stab_bytes = stab_point_bytes(stab);
        HIP_TRY(c->stab_ring.acquire(stab_bytes + 64, stream, &stab_slot), GFW_ERR_HIP);
        S = stab_device(stab, t->framebuffer_inverted ? -1.0 : 1.0, stab_slot->h.ptr, stab_slot->d.ptr);
        Sp = &S;
    }
    const size_t table_floats = (size_t)t->rows * GFW_MAT_STRIDE, table_bytes = table_floats * sizeof(float);
    float *table = rows16_out; double *prefix = nullptr;
    gfw_ctx::BuiltSlot *b = nullptr;
    if (rows16_out) {
        HIP_TRY(c->d_prefix.ensure(4 * sizeof(double)), GFW_ERR_HIP);
        prefix = (double *)c->d_prefix.ptr;
    } else {
        b = &c->bslots[c->bslot_next];
        c->bslot_next = (c->bslot_next + 1) % gfw_ctx::kBuiltSlots;
        HIP_TRY(b->buf.ensure(table_bytes + 4 * sizeof(double)), GFW_ERR_HIP);
        HIP_TRY(b->consumed.wait_on(stream), GFW_ERR_HIP);                   // the warp that read this slot is done
        table = (float *)b->buf.ptr; prefix = (double *)((char *)b->buf.ptr + table_bytes);
    }
    { const int rc = stage_timings(c, t, 1, stream, &t_slot); if (rc != GFW_OK) return rc; }
    if (stab_slot && stab_bytes) HIP_TRY(hipMemcpyAsync(stab_slot->d.ptr, stab_slot->h.ptr, stab_bytes, hipMemcpyHostToDevice, stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_build_matrices(c->tracks, (const gfw_frame_timing *)t_slot->d.ptr, 1, t->rows, prefix, table, table_floats, stream, Sp), GFW_ERR_HIP);
    if (b) HIP_TRY(b->built.record(stream), GFW_ERR_HIP);
    HIP_TRY(t_slot->free_again.record(stream), GFW_ERR_HIP);
    if (stab_slot) HIP_TRY(stab_slot->free_again.record(stream), GFW_ERR_HIP);
    if (out_ptr) *out_ptr = table;
    if (c->synchronous) HIP_TRY(hipStreamSynchronize(stream), GFW_ERR_HIP);
    return GFW_OK;
}
// The tables of `count` upcoming frames in one launch, in order on the context's stream: no cross-stream events, and the
// builder's latency (a few slerps in f64 per row) is paid once per batch instead of once per frame.
int gfw_build_matrices_batch(gfw_ctx *c, const gfw_frame_timing *t, int count, float **out_ptrs) {
    if (!c || !t || !out_ptrs || count < 1 || count > gfw_ctx::kMaxBatch) { set_error("bad batch arguments (1 <= count <= %d)", gfw_ctx::kMaxBatch); return GFW_ERR_INVALID_ARGUMENT; }
    int max_rows = 0;
    for (int i = 0; i < count; ++i) {
        if (!timing_ok(&t[i])) { set_error("frame %d: rows %d, readout_dim %d, suppress_rotation %d", i, t[i].rows, t[i].readout_dim, t[i].suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
        if (t[i].rows > max_rows) max_rows = t[i].rows;
    }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    // two batches alternate: the stream is in order, so the batch being overwritten was consumed by launches enqueued before this one (held frames have just left)
    DevBuf &buf = c->d_batch[c->batch_next];
    c->batch_next ^= 1;
    const size_t table_floats = (size_t)max_rows * GFW_MAT_STRIDE;
    const size_t tables_bytes = table_floats * sizeof(float) * count;
    HIP_TRY(buf.ensure(tables_bytes + 4 * sizeof(double) * count), GFW_ERR_HIP);
    StagingSlot *t_slot = nullptr;
    { const int rc = stage_timings(c, t, count, c->stream, &t_slot); if (rc != GFW_OK) return rc; }
    HIP_TRY(gfw_launch_build_matrices(c->tracks, (const gfw_frame_timing *)t_slot->d.ptr, count, max_rows, (double *)((char *)buf.ptr + tables_bytes), (float *)buf.ptr, table_floats, c->stream), GFW_ERR_HIP);
    HIP_TRY(t_slot->free_again.record(c->stream), GFW_ERR_HIP);
    for (int i = 0; i < count; ++i) out_ptrs[i] = (float *)buf.ptr + table_floats * i;
    if (c->synchronous) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
// The same for a clip with IBIS/OIS splines: frame i's table is gfw_build_matrices_stab(ctx, &t[i], stabs[i], ...)'s, bit for bit.  The descriptors of all frames and their
// control points go up in ONE pinned copy in front of the launch; the row kernel reads its frame's descriptor from that device table.
int gfw_build_matrices_batch_stab(gfw_ctx *c, const gfw_frame_timing *t, const gfw_frame_stab *const *stabs, int count, float **out_ptrs) {
    if (!stabs) return gfw_build_matrices_batch(c, t, count, out_ptrs);
    if (!c || !t || !out_ptrs || count < 1 || count > gfw_ctx::kMaxBatch) { set_error("bad batch arguments (1 <= count <= %d)", gfw_ctx::kMaxBatch); return GFW_ERR_INVALID_ARGUMENT; }
    int max_rows = 0;
    size_t point_bytes = 0;
    for (int i = 0; i < count; ++i) {
        if (!timing_ok(&t[i])) { set_error("frame %d: rows %d, readout_dim %d, suppress_rotation %d", i, t[i].rows, t[i].readout_dim, t[i].suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
        if (t[i].rows > max_rows) max_rows = t[i].rows;
        if (stabs[i]) { if (!stab_ok(stabs[i], i)) return GFW_ERR_INVALID_ARGUMENT; point_bytes += stab_point_bytes(stabs[i]); }
    }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    const size_t table_bytes = sizeof(GfwStab) * (size_t)count;
    StagingSlot *ss = nullptr, *t_slot = nullptr;
    HIP_TRY(c->stab_ring.acquire(table_bytes + point_bytes + 64, c->stream, &ss), GFW_ERR_HIP);
    GfwStab *h_stabs = (GfwStab *)ss->h.ptr;
    size_t at = table_bytes;
    for (int i = 0; i < count; ++i) {
        if (!stabs[i]) { h_stabs[i] = kNoStab; continue; }
        h_stabs[i] = stab_device(stabs[i], t[i].framebuffer_inverted ? -1.0 : 1.0, (char *)ss->h.ptr + at, (const char *)ss->d.ptr + at);
        at += stab_point_bytes(stabs[i]);
    }
    DevBuf &buf = c->d_batch[c->batch_next];
    c->batch_next ^= 1;
    const size_t table_floats = (size_t)max_rows * GFW_MAT_STRIDE;
    const size_t tables_bytes = table_floats * sizeof(float) * count;
    HIP_TRY(buf.ensure(tables_bytes + 4 * sizeof(double) * count), GFW_ERR_HIP);
    { const int rc = stage_timings(c, t, count, c->stream, &t_slot); if (rc != GFW_OK) return rc; }
    HIP_TRY(hipMemcpyAsync(ss->d.ptr, ss->h.ptr, at, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_build_matrices_stab(c->tracks, (const gfw_frame_timing *)t_slot->d.ptr, count, max_rows, (double *)((char *)buf.ptr + tables_bytes), (float *)buf.ptr, table_floats, c->stream, (const GfwStab *)ss->d.ptr), GFW_ERR_HIP);
    HIP_TRY(t_slot->free_again.record(c->stream), GFW_ERR_HIP);
    HIP_TRY(ss->free_again.record(c->stream), GFW_ERR_HIP);
    for (int i = 0; i < count; ++i) out_ptrs[i] = (float *)buf.ptr + table_floats * i;
    if (c->synchronous) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
}

// Inverse point map (`undistort_points`, cpu_undistort.rs:652-858; the STMap "dist"
// pass stmap.rs:123-127 runs it per pixel).  See include/gfwarp.h for the argument contract.
extern "C" int gfw_undistort_points(gfw_ctx *c, const gfw_kernel_params *p, const float *points, size_t n, int grid_width,
                                    const float *rotations, int rotation_count, const float *shifts, int index_mode,
                                    const double *mesh, size_t mesh_len, float *out, int out_on_device) {
    if (!c || !p || !rotations || !out || rotation_count < 1 || index_mode < 0 || index_mode > 3) { set_error("bad undistort_points arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!points && grid_width < 1) { set_error("grid_width must be >= 1 when points is NULL"); return GFW_ERR_INVALID_ARGUMENT; }
    if (mesh_len > GFW_MESH_MAX) { set_error("mesh too large"); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    { const int mrc = validate_mesh(mesh, mesh_len); if (mrc != GFW_OK) return mrc; }
    if (n == 0) return GFW_OK;                                               // :637 `if distorted.is_empty() { return Vec::new(); }`
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
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
    float *d_out = out;
    if (!out_on_device) { HIP_TRY(c->d_pts_out.ensure(pts_bytes), GFW_ERR_HIP); d_out = (float *)c->d_pts_out.ptr; }
    A.out = d_out;
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    HIP_TRY(gfw_launch_points(*p, C, A, c->stream), GFW_ERR_HIP);
    c->last_backend = "points";
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, d_out, pts_bytes, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
    // host staging vectors (packed shifts) and pageable copies: always complete before returning
    HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}

// STMap "undist" coordinate map (src/core/stmap.rs:87-109, :127-137): coords is width*height*2 f32, host or device
// memory (coords_on_device); pixels whose projection is None keep their previous content, as parallel_exr leaves 0.
extern "C" int gfw_stmap_undistort(gfw_ctx *c, const gfw_kernel_params *p, const float *matrices, int matrix_count,
                                   const float *mesh, size_t mesh_len, int width, int height, float *coords, int coords_on_device) {
    if (!c || !p || !coords || width < 1 || height < 1) { set_error("bad stmap arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    if (p->matrix_count != matrix_count || matrix_count < 1) { set_error("matrix_count %d != %d", p->matrix_count, matrix_count); return GFW_ERR_INVALID_ARGUMENT; }
    if (mesh_len > GFW_MESH_MAX) { set_error("mesh too large"); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    { const int mrc = validate_mesh(mesh, mesh_len); if (mrc != GFW_OK) return mrc; }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    const float *d_mat = nullptr;
    int rc = upload_matrices(c, matrices, matrix_count, &d_mat);
    if (rc != GFW_OK) return rc;
    const float *d_mesh = nullptr;
    if (mesh && mesh_len) { HIP_TRY(hipMemcpyAsync(c->d_mesh.ptr, mesh, mesh_len * sizeof(float), hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP); d_mesh = (const float *)c->d_mesh.ptr; }
    GfwCommon C;
    fill_common(c, p, d_mat, d_mesh, (int)mesh_len, C);
    const size_t bytes = (size_t)width * height * 2 * sizeof(float);
    float *d_coords = coords;
    if (!coords_on_device) {
        if (c->stage_dst.empty()) c->stage_dst.resize(1);
        HIP_TRY(c->stage_dst[0].ensure(bytes), GFW_ERR_HIP);
        d_coords = (float *)c->stage_dst[0].ptr;
        HIP_TRY(hipMemcpyAsync(d_coords, coords, bytes, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    }
    HIP_TRY(gfw_launch_stmap(*p, C, width, height, d_coords, c->stream), GFW_ERR_HIP);
    c->last_backend = "stmap";
    { const int mrc = matrices_consumed(c); if (mrc != GFW_OK) return mrc; }
    if (!coords_on_device) HIP_TRY(hipMemcpyAsync(coords, d_coords, bytes, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
    if (c->synchronous || !coords_on_device) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}

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
    size_t point_bytes = 0, mesh_doubles = 0;
    for (int i = 0; i < n_frames; ++i) {
        if (frames[i].suppress_rotation < 0 || frames[i].suppress_rotation > (with_data ? 2 : 1)) { set_error("frame %d: suppress_rotation %d", i, frames[i].suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
        if (rotations && frames[i].frame_readout_time_ms != 0.0) {
            set_error("frame %d: caller-given rotations are one per frame, but frame_readout_time_ms = %g needs one per point", i, frames[i].frame_readout_time_ms);
            return GFW_ERR_INVALID_ARGUMENT; }
        if (stabs && stabs[i]) { if (!stab_ok(stabs[i], i)) return GFW_ERR_INVALID_ARGUMENT; point_bytes += stab_point_bytes(stabs[i]); }
        if (meshes && mesh_lens[i]) {
            if (!meshes[i]) { set_error("frame %d: mesh of %zu values is NULL", i, mesh_lens[i]); return GFW_ERR_INVALID_ARGUMENT; }
            if (i && meshes[i] == meshes[i - 1] && mesh_lens[i] == mesh_lens[i - 1]) continue;            // the mesh of the frame before: checked and uploaded once
            if (mesh_lens[i] > GFW_MESH_MAX) { set_error("frame %d: mesh too large (%zu values, at most %d)", i, mesh_lens[i], GFW_MESH_MAX); return GFW_ERR_INVALID_ARGUMENT; }
            if (validate_mesh(meshes[i], mesh_lens[i]) != GFW_OK) { const std::string why = g_last_error; set_error("frame %d: %s", i, why.c_str()); return GFW_ERR_INVALID_ARGUMENT; }
            mesh_doubles += mesh_lens[i];
        }
    }
    if (mesh_doubles > 0x7fffffffu) { set_error("the clip's distinct meshes hold %zu values: more than a frame's 32-bit mesh reference addresses", mesh_doubles); return GFW_ERR_INVALID_ARGUMENT; }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    // descriptors (rotations, stabiliser tables, control points, meshes) through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    const size_t fb = sizeof(gfw_zoom_frame) * (size_t)n_frames, rb = rotations ? (sizeof(float) * 9 * (size_t)n_frames + 7) / 8 * 8 : 0;
    const size_t sb = stabs ? sizeof(GfwStab) * (size_t)n_frames : 0, mb = meshes ? sizeof(int32_t) * 2 * (size_t)n_frames : 0;
    const size_t o_stab = fb + rb, o_points = o_stab + sb, o_ref = o_points + point_bytes, o_mesh = o_ref + mb, total = o_mesh + mesh_doubles * sizeof(double);
    static_assert(sizeof(gfw_zoom_frame) % 8 == 0 && sizeof(GfwStab) % 8 == 0 && GFW_MESH_MAX == GFW_ZOOM_MESH_MAX, "the staged block keeps its doubles aligned; one mesh limit");
    StagingSlot *zs = nullptr;                                               // (free when the copy that last read the pinned block is done; a launch in flight that still
    HIP_TRY(c->zoom_ring.acquire(total, c->stream, &zs), GFW_ERR_HIP);       //  reads a device block about to be replaced is waited for)
    char *h = (char *)zs->h.ptr;
    const char *d = (const char *)zs->d.ptr;
    memcpy(h, frames, fb);
    if (rb) memcpy(h + fb, rotations, sizeof(float) * 9 * (size_t)n_frames);
    if (stabs) {
        GfwStab *hs = (GfwStab *)(h + o_stab);
        size_t at = o_points;
        for (int i = 0; i < n_frames; ++i) {
            if (!stabs[i]) { hs[i] = kNoStab; continue; }
            hs[i] = stab_device(stabs[i], 1.0, h + at, d + at);
            at += stab_point_bytes(stabs[i]);
        }
    }
    if (meshes) {
        int32_t *ref = (int32_t *)(h + o_ref);
        double *hm = (double *)(h + o_mesh);
        size_t at = 0, first = 0;
        for (int i = 0; i < n_frames; ++i) {
            if (!mesh_lens[i]) { ref[i * 2] = 0; ref[i * 2 + 1] = 0; continue; }
            if (!(i && meshes[i] == meshes[i - 1] && mesh_lens[i] == mesh_lens[i - 1])) { first = at; memcpy(hm + at, meshes[i], mesh_lens[i] * sizeof(double)); at += mesh_lens[i]; }
            ref[i * 2] = (int32_t)first; ref[i * 2 + 1] = (int32_t)mesh_lens[i];
        }
    }
    HIP_TRY(hipMemcpyAsync(zs->d.ptr, zs->h.ptr, total, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    HIP_TRY(zs->free_again.record(c->stream), GFW_ERR_HIP);
    const size_t ob = sizeof(double) * (size_t)n_frames, db = debug_points ? sizeof(double) * 2 * GFW_ZOOM_RECT * (size_t)n_frames : 0;
    double *d_fov = fov_minimal, *d_dbg = debug_points;
    if (!out_on_device) {
        HIP_TRY(c->d_zoom_out.ensure(ob + db), GFW_ERR_HIP);
        d_fov = (double *)c->d_zoom_out.ptr; d_dbg = debug_points ? d_fov + n_frames : nullptr;
    }
    GfwZoomArgs A;
    memset(&A, 0, sizeof(A));
    A.T = c->tracks;
    A.frames = (const gfw_zoom_frame *)d;
    A.rotations = rotations ? (const float *)(d + fb) : nullptr;
    if (stabs) A.stabs = (const GfwStab *)(d + o_stab);
    if (meshes) { A.mesh_ref = (const int32_t *)(d + o_ref); A.mesh_data = (const double *)(d + o_mesh); }
    A.fov_minimal = d_fov; A.debug_points = d_dbg;
    A.horizontal = search->horizontal_readout;
    A.w = (float)search->width; A.h = (float)search->height; A.margin = search->fov_algorithm_margin;
    // FovIterative::new (fov_iterative.rs:74-80), f32
    const float ratio = (float)search->width / (float)search->org_output_width;                  // (.max(1): validated >= 1)
    const float out_dim0 = (float)search->org_output_width * ratio, out_dim1 = (float)search->org_output_height * ratio;
    A.out_dim0 = out_dim0; A.inv_aspect = out_dim1 / out_dim0;
    A.readout_dim = search->horizontal_readout ? search->width : search->height;
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    HIP_TRY(gfw_launch_zoom(*p, C, A, n_frames, c->stream), GFW_ERR_HIP);
    c->last_backend = (stabs || meshes) ? "zoom_fovs_stab" : "zoom_fovs";
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(fov_minimal, d_fov, ob, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
        if (db) HIP_TRY(hipMemcpyAsync(debug_points, d_dbg, db, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
    }
    if (c->synchronous || !out_on_device) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
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

// Adaptive zoom, second half, on the host: zooming/mod.rs:55-68 and zoom_dynamic.rs in f64, the reference's operation order.
static int zoom_frames_per_window(double window, double fps) {               // zoom_dynamic.rs:84-90 (`as usize` saturates; NaN -> 0)
    const double v = floor(window * fps);
    long long frames = !(v == v) || v <= 0.0 ? 0 : (v >= 1e9 ? 1000000000LL : (long long)v);
    if (frames % 2 == 0) frames += 1;
    return (int)frames;
}
static std::vector<double> zoom_pad_edge(const std::vector<double> &a, size_t before, size_t after) {       // :119-131
    std::vector<double> out(a.size() + before + after, 0.0);
    const double first = a.empty() ? 0.0 : a.front(), last = a.empty() ? 0.0 : a.back();
    for (size_t i = 0; i < a.size(); ++i) out[before + i] = a[i];
    for (size_t i = 0; i < before; ++i) out[i] = first;
    for (size_t i = before + a.size(); i < out.size(); ++i) out[i] = last;
    return out;
}
static std::vector<double> zoom_envelope_follower(const std::vector<double> &a, double alpha) {             // :170-194 with a constant alpha
    const size_t n = a.size();
    std::vector<double> rev(n), out(n);
    if (!n) return out;
    double q = a[n - 1];
    for (size_t k = 0; k < n; ++k) { const double x = a[n - 1 - k]; q = fmin(x, x * alpha + q * (1.0 - alpha)); rev[k] = q; }      // smoothed_rev, in reversed order
    q = rev[n - 1];
    for (size_t k = 0; k < n; ++k) { const double x = rev[n - 1 - k]; q = fmin(x, x * alpha + q * (1.0 - alpha)); out[k] = q; }
    return out;
}
extern "C" int gfw_zoom_smooth(const double *fov_minimal, int n, double adaptive_zoom_window, double scaled_fps, int method,
                               const double *trim_ranges, int n_ranges, double *fovs_out, double *fov_minimal_out) {
    if (n < 0 || n_ranges < 0 || (n && (!fov_minimal || !fovs_out)) || (n_ranges && !trim_ranges) || !(adaptive_zoom_window == adaptive_zoom_window)) {
        set_error("bad zoom_smooth arguments (n %d, n_ranges %d, window %g)", n, n_ranges, adaptive_zoom_window); return GFW_ERR_INVALID_ARGUMENT; }
    if (adaptive_zoom_window > 0.0001 && !(scaled_fps > 0.0)) { set_error("scaled_fps %g", scaled_fps); return GFW_ERR_INVALID_ARGUMENT; }
    if (n == 0) return GFW_OK;
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
    return GFW_OK;
}

// The visual-features sync search (find_offset/visual_features.rs:10-147; gfw_sync.hip).  See include/gfwarp.h for the argument contract.  One body serves both entries:
// `search_mode` < 0 = gfw_sync_visual_costs (the caller's candidates), 0 / 1 = gfw_sync_visual_search (the coarse candidates are made here, the fine ones on the device).
struct SyncOut { double *costs; float *mapped; gfw_sync_result *result; double *coarse_costs, *fine_costs; };
static int sync_visual_impl(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_search *search, const int64_t *pair_ts_us, const int32_t *pair_first,
                            const float *points_a, const float *points_b, int n_pairs, const double *candidates, int n_candidates, int search_mode,
                            double initial_offset_ms, double search_size_ms, double frame_readout_time_ms, double scaled_fps, const SyncOut &out, int out_on_device) {
    if (!c || !p || !search || n_pairs < 0 || n_candidates < 0) { set_error("bad sync arguments (null context / params / search, or a negative count)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (search->reserved[0] || search->reserved[1]) { set_error("bad sync search: reserved slots must be 0"); return GFW_ERR_INVALID_ARGUMENT; }
    if (search->width < 1 || search->height < 1 || search->horizontal_readout < 0 || search->horizontal_readout > 1 || search->use_sync_offsets < 0 || search->use_sync_offsets > 1) {
        set_error("bad sync search: %d x %d, horizontal_readout %d, use_sync_offsets %d", search->width, search->height, search->horizontal_readout, search->use_sync_offsets);
        return GFW_ERR_INVALID_ARGUMENT; }
    if ((unsigned long long)search->width * (unsigned long long)search->width + (unsigned long long)search->height * (unsigned long long)search->height >= (1ull << 32)) {
        set_error("bad sync search: %d x %d — width^2 + height^2 must stay below 2^32 (a squared distance is folded as 32 bits)", search->width, search->height);
        return GFW_ERR_INVALID_ARGUMENT; }
    if (p->flags & (256 | 512 | 1024)) {                                     // HAS_IBIS_DATA | HAS_MESH_DATA | HAS_FPD_DATA
        set_error("the sync search does not cover per-frame IBIS/OIS shifts, lens meshes or focal-plane distortion data (flags 0x%x)", p->flags);
        return GFW_ERR_INVALID_ARGUMENT; }
    if (n_pairs > GFW_SYNC_PAIRS_MAX) { set_error("%d pairs: at most %d in a call", n_pairs, GFW_SYNC_PAIRS_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_pairs && (!pair_ts_us || !pair_first)) { set_error("bad sync arguments (pairs without pair_ts_us / pair_first)"); return GFW_ERR_INVALID_ARGUMENT; }
    int total = 0, max_pair = 0;
    if (n_pairs) {
        if (pair_first[0] < 0) { set_error("pair 0: pair_first %d is negative", pair_first[0]); return GFW_ERR_INVALID_ARGUMENT; }
        for (int i = 0; i < n_pairs; ++i) {
            if (pair_first[i + 1] < pair_first[i]) { set_error("pair %d: pair_first descends (%d after %d)", i, pair_first[i + 1], pair_first[i]); return GFW_ERR_INVALID_ARGUMENT; }
            const int n = pair_first[i + 1] - pair_first[i];
            if (n > GFW_SYNC_PAIR_MAX) { set_error("pair %d: %d points, at most %d", i, n, GFW_SYNC_PAIR_MAX); return GFW_ERR_INVALID_ARGUMENT; }
            if (n > max_pair) max_pair = n;
        }
        total = pair_first[n_pairs];
        if (total && (!points_a || !points_b)) { set_error("bad sync arguments (%d points without points_a / points_b)", total); return GFW_ERR_INVALID_ARGUMENT; }
    }
    int n_coarse = n_candidates;
    if (search_mode < 0) {
        if (n_candidates && (!candidates || !out.costs)) { set_error("bad sync arguments (candidates without their array / costs)"); return GFW_ERR_INVALID_ARGUMENT; }
    } else {
        if (search_mode > 1 || !out.result) { set_error("bad sync arguments (mode %d, or a null result)", search_mode); return GFW_ERR_INVALID_ARGUMENT; }
        // `search_size as usize` (:113) / `(1000.0 / fps) as isize`, `-steps..steps` (:89-91): saturating casts, NaN -> 0
        const double v = search_mode == 0 ? search_size_ms : 1000.0 / scaled_fps;
        const double steps = !(v == v) || v <= 0.0 ? 0.0 : trunc(v);
        if (steps > 1000000.0) { set_error("a search of %g candidates (search_size_ms %g, scaled_fps %g)", steps * (search_mode ? 2.0 : 1.0), search_size_ms, scaled_fps); return GFW_ERR_INVALID_ARGUMENT; }
        n_coarse = (int)steps * (search_mode ? 2 : 1);
    }
    if (c->tracks.org_n < 1 && c->tracks.sm_n < 1) { set_error("no quaternion tracks set (gfw_set_quaternion_tracks)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (search_mode < 0 && n_candidates == 0) return GFW_OK;
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    // pairs, points and candidates through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    const size_t tb = sizeof(int64_t) * 2 * (size_t)n_pairs, fb = (sizeof(int32_t) * ((size_t)n_pairs + 1) + 7) / 8 * 8, pb = sizeof(float) * 2 * (size_t)total;
    const size_t cb = sizeof(double) * 2 * (size_t)n_coarse;
    const size_t o_first = tb, o_pts = o_first + fb, o_cand = o_pts + pb * 2, staged = o_cand + cb;
    StagingSlot *ss = nullptr;
    HIP_TRY(c->sync_ring.acquire(staged + 8, c->stream, &ss), GFW_ERR_HIP);
    char *h = (char *)ss->h.ptr;
    const char *d = (const char *)ss->d.ptr;
    if (n_pairs) { memcpy(h, pair_ts_us, tb); memcpy(h + o_first, pair_first, sizeof(int32_t) * ((size_t)n_pairs + 1)); }
    else *(int32_t *)(h + o_first) = 0;
    if (total) { memcpy(h + o_pts, points_a, pb); memcpy(h + o_pts + pb, points_b, pb); }
    double *hc = (double *)(h + o_cand);
    if (search_mode < 0) memcpy(hc, candidates, cb);
    else for (int i = 0; i < n_coarse; ++i) {
        if (search_mode == 0) { hc[i * 2] = initial_offset_ms + (-(search_size_ms / 2.0) + (double)i); hc[i * 2 + 1] = frame_readout_time_ms; }
        else { hc[i * 2] = 0.0; hc[i * 2 + 1] = (double)(i - n_coarse / 2); }
    }
    HIP_TRY(hipMemcpyAsync(ss->d.ptr, ss->h.ptr, staged + 8, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    HIP_TRY(ss->free_again.record(c->stream), GFW_ERR_HIP);
    // device work space: rays, partials of the larger stage, the fine candidates
    const int n_wide = search_mode < 0 ? n_coarse : (n_coarse > GFW_SYNC_FINE ? n_coarse : GFW_SYNC_FINE);
    const size_t rb = sizeof(float4) * 2 * (size_t)total, qb = sizeof(unsigned long long) * (size_t)n_wide * (size_t)(n_pairs ? n_pairs : 1), eb = sizeof(double) * 2 * GFW_SYNC_FINE;
    HIP_TRY(c->d_sync_work.ensure(rb + qb + eb + 16), GFW_ERR_HIP);
    char *wk = (char *)c->d_sync_work.ptr;
    // outputs: the caller's device memory, or the context's to be copied back
    const size_t res_b = 48, cc_b = sizeof(double) * (size_t)n_coarse, fc_b = sizeof(double) * GFW_SYNC_FINE;
    const size_t map_b = out.mapped ? sizeof(float) * 4 * (size_t)total * (size_t)n_coarse : 0;
    double *d_costs = search_mode < 0 ? out.costs : out.coarse_costs, *d_fine_costs = out.fine_costs;
    float *d_mapped = out.mapped; gfw_sync_result *d_result = out.result;
    if (!out_on_device) {
        HIP_TRY(c->d_sync_out.ensure(res_b + cc_b + fc_b + map_b + 16), GFW_ERR_HIP);
        char *ob = (char *)c->d_sync_out.ptr;
        d_result = out.result ? (gfw_sync_result *)ob : nullptr;
        d_costs = d_costs ? (double *)(ob + res_b) : nullptr;
        d_fine_costs = d_fine_costs ? (double *)(ob + res_b + cc_b) : nullptr;
        d_mapped = out.mapped ? (float *)(ob + res_b + cc_b + fc_b) : nullptr;
    }
    GfwSyncArgs A;
    memset(&A, 0, sizeof(A));
    A.T = c->tracks;
    if (!search->use_sync_offsets) { A.T.off_ts = nullptr; A.T.off_ms = nullptr; A.T.off_n = 0; }      // clear_offsets()
    for (int i = 0; i < 9; ++i) A.F.new_k[i] = search->new_k[i];
    A.F.video_rotation_deg = search->video_rotation_deg;
    A.pair_ts = (const int64_t *)d; A.pair_first = (const int32_t *)(d + o_first); A.points = (const float *)(d + o_pts);
    A.rays = (float4 *)wk; A.partial = (unsigned long long *)(wk + rb);
    A.candidates = (const double *)(d + o_cand); A.mapped = d_mapped;
    A.w = (float)search->width; A.h = (float)search->height;
    A.horizontal = search->horizontal_readout; A.readout_dim = search->horizontal_readout ? search->width : search->height;
    A.n_pairs = n_pairs; A.total = total;
    GfwCommon C;
    fill_common(c, p, nullptr, nullptr, 0, C);
    GfwSyncReduceArgs R;
    memset(&R, 0, sizeof(R));
    R.partial = A.partial; R.candidates = A.candidates; R.costs = d_costs; R.result = d_result; R.fine = (double *)(wk + rb + qb);
    R.n = n_coarse; R.n_pairs = n_pairs; R.column = search_mode == 1 ? 1 : 0; R.stage = 0;
    HIP_TRY(gfw_launch_sync_rays(*p, C, A, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_sync_costs(A, n_coarse, max_pair, c->stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_sync_reduce(R, c->stream), GFW_ERR_HIP);
    if (search_mode >= 0) {
        A.candidates = R.fine; A.gate = d_result; A.mapped = nullptr;
        HIP_TRY(gfw_launch_sync_costs(A, GFW_SYNC_FINE, max_pair, c->stream), GFW_ERR_HIP);
        R.candidates = R.fine; R.costs = d_fine_costs; R.n = GFW_SYNC_FINE; R.stage = 1;
        HIP_TRY(gfw_launch_sync_reduce(R, c->stream), GFW_ERR_HIP);
    }
    c->last_backend = search_mode < 0 ? "sync_visual_costs" : "sync_visual_search";
    if (!out_on_device) {
        if (out.result) HIP_TRY(hipMemcpyAsync(out.result, d_result, sizeof(gfw_sync_result), hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
        if (d_costs && cc_b) HIP_TRY(hipMemcpyAsync(search_mode < 0 ? out.costs : out.coarse_costs, d_costs, cc_b, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
        if (d_fine_costs) HIP_TRY(hipMemcpyAsync(out.fine_costs, d_fine_costs, fc_b, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
        if (map_b) HIP_TRY(hipMemcpyAsync(out.mapped, d_mapped, map_b, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
    }
    if (c->synchronous || !out_on_device) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
extern "C" int gfw_sync_visual_costs(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_search *search, const int64_t *pair_ts_us, const int32_t *pair_first,
                                     const float *points_a, const float *points_b, int n_pairs, const double *candidates, int n_candidates,
                                     double *costs, float *mapped, int out_on_device) {
    const SyncOut out = {costs, mapped, nullptr, nullptr, nullptr};
    return sync_visual_impl(c, p, search, pair_ts_us, pair_first, points_a, points_b, n_pairs, candidates, n_candidates, -1, 0.0, 0.0, 0.0, 0.0, out, out_on_device);
}
extern "C" int gfw_sync_visual_search(gfw_ctx *c, const gfw_kernel_params *p, const gfw_sync_search *search, const int64_t *pair_ts_us, const int32_t *pair_first,
                                      const float *points_a, const float *points_b, int n_pairs, int mode, double initial_offset_ms, double search_size_ms,
                                      double frame_readout_time_ms, double scaled_fps, gfw_sync_result *result, double *coarse_costs, double *fine_costs, int out_on_device) {
    const SyncOut out = {nullptr, nullptr, result, coarse_costs, fine_costs};
    return sync_visual_impl(c, p, search, pair_ts_us, pair_first, points_a, points_b, n_pairs, nullptr, 0, mode < 0 ? 2 : mode, initial_offset_ms, search_size_ms,
                            frame_readout_time_ms, scaled_fps, out, out_on_device);
}

// Lowpass::filter_gyro_forward_backward (filtering.rs:46-74) of a gyro triple series, in place: biquad's second-order Butterworth low-pass (Q = FRAC_1_SQRT_2) in
// transposed direct form II, forward then backward, one filter per axis and direction; entries without a gyro do not advance the state.  See include/gfwarp.h.
extern "C" int gfw_lowpass_gyro(double freq, double sample_rate, double *xyz, const uint8_t *has, int n) {
    if (n < 0 || (n && !xyz)) { set_error("bad lowpass arguments (n %d)", n); return GFW_ERR_INVALID_ARGUMENT; }
    // Coefficients::from_params fails for 2 f0 > fs (and the reference ignores the failure: essential_matrix.rs:47-48)
    if (!std::isfinite(freq) || !std::isfinite(sample_rate) || !(freq > 0.0) || !(sample_rate > 0.0) || 2.0 * freq > sample_rate) return GFW_FILTER_NOT_APPLIED;
    const double omega = 2.0 * 3.14159265358979323846 * freq / sample_rate;
    const double omega_s = sin(omega), omega_c = cos(omega);
    const double alpha = omega_s / (2.0 * 0.70710678118654752440);
    const double b0 = (1.0 - omega_c) * 0.5, b1 = 1.0 - omega_c, b2 = (1.0 - omega_c) * 0.5;
    const double a0 = 1.0 + alpha, a1 = -2.0 * omega_c, a2 = 1.0 - alpha;
    const double cb0 = b0 / a0, cb1 = b1 / a0, cb2 = b2 / a0, ca1 = a1 / a0, ca2 = a2 / a0;
    for (int pass = 0; pass < 2; ++pass) {
        double s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < n; ++k) {
            const int i = pass ? n - 1 - k : k;
            if (has && !has[i]) continue;
            for (int a = 0; a < 3; ++a) {
                const double x = xyz[(size_t)i * 3 + a];
                const double out = s1[a] + cb0 * x;
                s1[a] = s2[a] + cb1 * x - ca1 * out;
                s2[a] = cb2 * x - ca2 * out;
                xyz[(size_t)i * 3 + a] = out;
            }
        }
    }
    return GFW_OK;
}

// The gyro-match sync search (find_offset/essential_matrix.rs:52-75, :109-131; gfw_sync_gyro.hip).  See include/gfwarp.h for the argument contract.  One body serves
// both entries: `search` false = gfw_sync_gyro_costs (the caller's candidates), true = gfw_sync_gyro_search (the coarse candidates are made here, the fine ones on the device).
struct GyroSeries { const int32_t *first; const double *data; const uint8_t *has; int total; const char *what; int limit; };
static bool gyro_series_ok(const GyroSeries &s, int n_ranges, bool needs_data = true) {
    if (!s.first || s.total < 0) { set_error("bad sync arguments (%s: a null first array, or a negative length %d)", s.what, s.total); return false; }
    if (s.first[0] < 0) { set_error("range 0: %s first %d is negative", s.what, s.first[0]); return false; }
    for (int r = 0; r < n_ranges; ++r) {
        if (s.first[r + 1] < s.first[r]) { set_error("range %d: %s first descends (%d after %d)", r, s.what, s.first[r + 1], s.first[r]); return false; }
        if (s.first[r + 1] > s.total) { set_error("range %d: %s slice %d .. %d lies outside its array of %d", r, s.what, s.first[r], s.first[r + 1], s.total); return false; }
        if (s.first[r + 1] - s.first[r] > s.limit) { set_error("range %d: %d %s, at most %d", r, s.first[r + 1] - s.first[r], s.what, s.limit); return false; }
    }
    if (needs_data && s.first[n_ranges] > 0 && !s.data) { set_error("bad sync arguments (%d %s without their array)", s.first[n_ranges], s.what); return false; }
    return true;
}
static int sync_gyro_impl(gfw_ctx *c, const GyroSeries &est, const GyroSeries &gyro, int n_ranges, const GyroSeries &cand, bool search,
                          double initial_offset_ms, double search_size_ms, double *costs, gfw_sync_result *results, double *coarse_costs, double *fine_costs, int out_on_device) {
    if (!c || n_ranges < 0) { set_error("bad sync arguments (null context, or a negative range count)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_ranges > GFW_GYRO_RANGES_MAX) { set_error("%d ranges: at most %d in a call", n_ranges, GFW_GYRO_RANGES_MAX); return GFW_ERR_INVALID_ARGUMENT; }
    size_t n_coarse = 0;
    if (search) {
        if (!std::isfinite(initial_offset_ms) || !std::isfinite(search_size_ms) || search_size_ms < 0.0) {
            set_error("bad sync search: initial_offset_ms %g, search_size_ms %g", initial_offset_ms, search_size_ms); return GFW_ERR_INVALID_ARGUMENT; }
        if (search_size_ms * 2.0 > (double)GFW_GYRO_COARSE_MAX) { set_error("a search of %g candidates a range (search_size_ms %g), at most %d", trunc(search_size_ms) * 2.0, search_size_ms, GFW_GYRO_COARSE_MAX); return GFW_ERR_INVALID_ARGUMENT; }
        n_coarse = (size_t)search_size_ms * 2;                              // `search_size as usize * 2` (:55): the cast comes first
        if (n_ranges && !results) { set_error("bad sync arguments (a null result array)"); return GFW_ERR_INVALID_ARGUMENT; }
    } else if (n_ranges && !costs) { set_error("bad sync arguments (a null cost array)"); return GFW_ERR_INVALID_ARGUMENT; }
    if (n_ranges == 0) return GFW_OK;
    if (!gyro_series_ok(est, n_ranges) || !gyro_series_ok(gyro, n_ranges) || (!search && !gyro_series_ok(cand, n_ranges))) return GFW_ERR_INVALID_ARGUMENT;
    const size_t tot_est = (size_t)est.first[n_ranges] - (size_t)est.first[0], tot_gyro = (size_t)gyro.first[n_ranges] - (size_t)gyro.first[0];
    const size_t tot_cand = search ? n_coarse * (size_t)n_ranges : (size_t)cand.first[n_ranges] - (size_t)cand.first[0];
    const size_t o_est = sizeof(GfwGyroRange) * (size_t)n_ranges, o_has = o_est + 32 * tot_est, o_keys = o_has + (tot_est + 7) / 8 * 8, o_val = o_keys + 8 * tot_gyro;
    const size_t o_cand = o_val + 32 * tot_gyro, staged = o_cand + 8 * tot_cand + 8;
    if (staged > ((size_t)1 << 31)) { set_error("the call stages %zu bytes (%zu estimated samples, %zu gyro samples, %zu candidates): at most 2 GiB", staged, tot_est, tot_gyro, tot_cand); return GFW_ERR_INVALID_ARGUMENT; }
    if (!search && tot_cand == 0) return GFW_OK;
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }
    HIP_TRY(hipSetDevice(c->device), GFW_ERR_HIP);
    // everything through pinned memory in one copy: it is enqueued, the caller's arrays are free on return
    StagingSlot *ss = nullptr;
    HIP_TRY(c->gyro_ring.acquire(staged, c->stream, &ss), GFW_ERR_HIP);
    char *h = (char *)ss->h.ptr;
    const char *d = (const char *)ss->d.ptr;
    GfwGyroRange *hr = (GfwGyroRange *)h;
    double *h_est = (double *)(h + o_est), *h_val = (double *)(h + o_val), *h_cand = (double *)(h + o_cand);
    uint8_t *h_has = (uint8_t *)(h + o_has);
    unsigned long long *h_keys = (unsigned long long *)(h + o_keys);
    const GfwGyroSeries se = {est.first, est.data, est.has}, sg = {gyro.first, gyro.data, gyro.has};
    const int max_cand = gfw_gyro_stage(se, sg, n_ranges, search ? nullptr : cand.first, cand.data, n_coarse, initial_offset_ms, search_size_ms, hr, h_est, h_has, h_keys, h_val, h_cand);
    HIP_TRY(hipMemcpyAsync(ss->d.ptr, ss->h.ptr, staged, hipMemcpyHostToDevice, c->stream), GFW_ERR_HIP);
    // outputs: the caller's device memory, or the context's to be copied back; what the caller does not ask for lives in the work space
    const size_t res_b = (sizeof(gfw_sync_result) * (size_t)n_ranges + 7) / 8 * 8, cc_b = 8 * tot_cand, fc_b = 8 * GFW_GYRO_FINE * (size_t)n_ranges;
    // caller-given candidates: range r's costs are the caller's entries cand_first[r] ..; the staged ranges count from 0, so the base moves by cand_first[0]
    double *const costs_out = search ? coarse_costs : costs + cand.first[0];
    double *d_costs = costs_out, *d_fine_costs = fine_costs;
    gfw_sync_result *d_results = results;
    if (!out_on_device) {
        HIP_TRY(c->d_sync_out.ensure(res_b + cc_b + fc_b + 16), GFW_ERR_HIP);
        char *ob = (char *)c->d_sync_out.ptr;
        d_results = (gfw_sync_result *)ob;
        d_costs = d_costs ? (double *)(ob + res_b) : nullptr;
        d_fine_costs = d_fine_costs ? (double *)(ob + res_b + cc_b) : nullptr;
    }
    HIP_TRY(c->d_sync_work.ensure(fc_b * 2 + cc_b + 16), GFW_ERR_HIP);
    double *wk = (double *)c->d_sync_work.ptr;
    GfwGyroArgs A;
    memset(&A, 0, sizeof(A));
    A.ranges = (const GfwGyroRange *)d; A.est = (const double *)(d + o_est); A.est_has = (const uint8_t *)(d + o_has);
    A.keys = (const unsigned long long *)(d + o_keys); A.gyro = (const double *)(d + o_val);
    A.candidates = (const double *)(d + o_cand); A.costs = d_costs ? d_costs : wk + 2 * GFW_GYRO_FINE * (size_t)n_ranges; A.stage = 0;
    HIP_TRY(gfw_launch_gyro_costs(A, n_ranges, max_cand, c->stream), GFW_ERR_HIP);
    if (search) {
        GfwGyroPickArgs R;
        memset(&R, 0, sizeof(R));
        R.ranges = A.ranges; R.candidates = A.candidates; R.costs = A.costs; R.results = d_results; R.fine = wk; R.stage = 0;
        HIP_TRY(gfw_launch_gyro_pick(R, n_ranges, c->stream), GFW_ERR_HIP);
        A.candidates = wk; A.costs = d_fine_costs ? d_fine_costs : wk + GFW_GYRO_FINE * (size_t)n_ranges; A.gate = d_results; A.stage = 1;
        HIP_TRY(gfw_launch_gyro_costs(A, n_ranges, GFW_GYRO_FINE, c->stream), GFW_ERR_HIP);
        R.candidates = wk; R.costs = A.costs; R.fine_costs = d_fine_costs; R.stage = 1;
        HIP_TRY(gfw_launch_gyro_pick(R, n_ranges, c->stream), GFW_ERR_HIP);
    }
    HIP_TRY(ss->free_again.record(c->stream), GFW_ERR_HIP);                 // behind the last launch that reads the slot's device side
    c->last_backend = search ? "sync_gyro_search" : "sync_gyro_costs";
    if (!out_on_device) {
        if (search) HIP_TRY(hipMemcpyAsync(results, d_results, sizeof(gfw_sync_result) * (size_t)n_ranges, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
        if (d_costs && cc_b) HIP_TRY(hipMemcpyAsync(costs_out, d_costs, cc_b, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
        if (d_fine_costs) HIP_TRY(hipMemcpyAsync(fine_costs, d_fine_costs, fc_b, hipMemcpyDeviceToHost, c->stream), GFW_ERR_HIP);
    }
    if (c->synchronous || !out_on_device) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
extern "C" int gfw_sync_gyro_costs(gfw_ctx *c, const int32_t *est_first, const double *est, const uint8_t *est_has, int n_est,
                                   const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has, int n_gyro, int n_ranges,
                                   const int32_t *cand_first, const double *candidates, int n_candidates, double *costs, int out_on_device) {
    const GyroSeries e = {est_first, est, est_has, n_est, "estimated samples", GFW_GYRO_EST_MAX}, g = {gyro_first, gyro, gyro_has, n_gyro, "gyro samples", GFW_GYRO_SAMPLES_MAX};
    const GyroSeries k = {cand_first, candidates, nullptr, n_candidates, "candidates", GFW_GYRO_COARSE_MAX};
    return sync_gyro_impl(c, e, g, n_ranges, k, false, 0.0, 0.0, costs, nullptr, nullptr, nullptr, out_on_device);
}
extern "C" int gfw_sync_gyro_search(gfw_ctx *c, const int32_t *est_first, const double *est, const uint8_t *est_has, int n_est,
                                    const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has, int n_gyro, int n_ranges,
                                    double initial_offset_ms, double search_size_ms, gfw_sync_result *results, double *coarse_costs, double *fine_costs, int out_on_device) {
    const GyroSeries e = {est_first, est, est_has, n_est, "estimated samples", GFW_GYRO_EST_MAX}, g = {gyro_first, gyro, gyro_has, n_gyro, "gyro samples", GFW_GYRO_SAMPLES_MAX};
    const GyroSeries k = {nullptr, nullptr, nullptr, 0, "candidates", GFW_GYRO_COARSE_MAX};
    return sync_gyro_impl(c, e, g, n_ranges, k, true, initial_offset_ms, search_size_ms, nullptr, results, coarse_costs, fine_costs, out_on_device);
}
