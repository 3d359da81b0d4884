// gfw_api_matrices.inc — part of gfw_api.hip (textually included): the per-row matrix builder's entry points (SURVEY.md section 8f) — gfw_set_quaternion_tracks,
// gfw_set_sync_offsets, gfw_build_matrices*.  The device form of the stabiliser data is gfw_matrices_host.h's.

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
static int stage_timings(gfw_ctx *c, const gfw_frame_timing *t, int count, hipStream_t stream, StagedBlock *out) {
    const size_t slot_bytes = sizeof(gfw_frame_timing) * gfw_ctx::kMaxBatch;
    if (!c->timing_ring.slots[0].d.ptr) HIP_TRY(c->timing_ring.reserve(slot_bytes), GFW_ERR_HIP);
    HIP_TRY(c->timing_ring.acquire(slot_bytes, stream, &out->slot), GFW_ERR_HIP);
    memcpy(out->h(), t, sizeof(gfw_frame_timing) * count);
    HIP_TRY(out->upload(sizeof(gfw_frame_timing) * count, stream), GFW_ERR_HIP);
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

int gfw_build_matrices(gfw_ctx *c, const gfw_frame_timing *t, float *rows16_out, float **out_ptr) {
    return gfw_build_matrices_stab(c, t, nullptr, rows16_out, out_ptr);
}
int gfw_build_matrices_stab(gfw_ctx *c, const gfw_frame_timing *t, const gfw_frame_stab *stab, float *rows16_out, float **out_ptr) {
    if (!c || !t) { set_error("null context/timing"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!timing_ok(t)) { set_error("rows %d, readout_dim %d, suppress_rotation %d", t->rows, t->readout_dim, t->suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
    API_TRY(enter_device(c));
    if (stab && !stab_ok(stab, -1)) return GFW_ERR_INVALID_ARGUMENT;
    // a caller-owned table is built in order on the context's stream; a context-owned one in the next slot of the ring, on the auxiliary stream (overlaps the warp in flight)
    const hipStream_t stream = rows16_out ? c->stream : c->copy_stream;
    GfwStab S, *Sp = nullptr;
    StagedBlock sb, tb;
    const size_t stab_bytes = stab ? stab_point_bytes(stab) : 0;
    if (stab) {
        HIP_TRY(c->stab_ring.acquire(stab_bytes + 64, stream, &sb.slot), GFW_ERR_HIP);
        S = stab_device(stab, t->framebuffer_inverted ? -1.0 : 1.0, sb.h(), sb.d());
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
    API_TRY(stage_timings(c, t, 1, stream, &tb));
    if (stab_bytes) HIP_TRY(sb.upload(stab_bytes, stream), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_build_matrices(c->tracks, (const gfw_frame_timing *)tb.d(), 1, t->rows, prefix, table, table_floats, stream, Sp), GFW_ERR_HIP);
    if (b) HIP_TRY(b->built.record(stream), GFW_ERR_HIP);
    HIP_TRY(tb.free_again(stream), GFW_ERR_HIP);
    if (stab) HIP_TRY(sb.free_again(stream), GFW_ERR_HIP);
    if (out_ptr) *out_ptr = table;
    if (c->synchronous) HIP_TRY(hipStreamSynchronize(stream), GFW_ERR_HIP);
    return GFW_OK;
}
// The tables of `count` upcoming frames in one launch, in order on the context's stream: no cross-stream events, and the builder's latency (a few slerps in f64 per
// row) is paid once per batch instead of once per frame.  `stabs`: NULL (the plain row kernel), or a clip with IBIS/OIS splines — frame i's table is
// gfw_build_matrices_stab(ctx, &t[i], stabs[i], ...)'s, bit for bit: the descriptors of all frames and their control points go up in ONE pinned copy in front of the
// launch, the row kernel reads its frame's descriptor from that device table.
int gfw_build_matrices_batch_stab(gfw_ctx *c, const gfw_frame_timing *t, const gfw_frame_stab *const *stabs, int count, float **out_ptrs) {
    if (!c || !t || !out_ptrs || count < 1 || count > gfw_ctx::kMaxBatch) { set_error("bad batch arguments (1 <= count <= %d)", gfw_ctx::kMaxBatch); return GFW_ERR_INVALID_ARGUMENT; }
    int max_rows = 0;
    for (int i = 0; i < count; ++i) {
        if (!timing_ok(&t[i])) { set_error("frame %d: rows %d, readout_dim %d, suppress_rotation %d", i, t[i].rows, t[i].readout_dim, t[i].suppress_rotation); return GFW_ERR_INVALID_ARGUMENT; }
        if (t[i].rows > max_rows) max_rows = t[i].rows;
        if (stabs && stabs[i] && !stab_ok(stabs[i], i)) return GFW_ERR_INVALID_ARGUMENT;
    }
    API_TRY(enter_device(c));
    StagedBlock sb, tb;
    const GfwStab *d_stabs = nullptr;
    BlockLayout L;
    if (stabs) {
        const GfwStabTable S = gfw_stab_table_layout(L, count, gfw_stab_points_total(stabs, count));
        HIP_TRY(c->stab_ring.acquire(L.total + 64, c->stream, &sb.slot), GFW_ERR_HIP);
        d_stabs = gfw_stab_table_fill(S, stabs, t, count, sb.h(), sb.d());
    }
    // two batches alternate: the stream is in order, so the batch being overwritten was consumed by launches enqueued before this one (held frames have just left)
    DevBuf &buf = c->d_batch[c->batch_next];
    c->batch_next ^= 1;
    const size_t table_floats = (size_t)max_rows * GFW_MAT_STRIDE;
    const size_t tables_bytes = table_floats * sizeof(float) * count;
    HIP_TRY(buf.ensure(tables_bytes + 4 * sizeof(double) * count), GFW_ERR_HIP);
    double *prefix = (double *)((char *)buf.ptr + tables_bytes);
    API_TRY(stage_timings(c, t, count, c->stream, &tb));
    const gfw_frame_timing *d_t = (const gfw_frame_timing *)tb.d();
    if (stabs) {
        HIP_TRY(sb.upload(L.total, c->stream), GFW_ERR_HIP);
        HIP_TRY(gfw_launch_build_matrices_stab(c->tracks, d_t, count, max_rows, prefix, (float *)buf.ptr, table_floats, c->stream, d_stabs), GFW_ERR_HIP);
    } else HIP_TRY(gfw_launch_build_matrices(c->tracks, d_t, count, max_rows, prefix, (float *)buf.ptr, table_floats, c->stream), GFW_ERR_HIP);
    HIP_TRY(tb.free_again(c->stream), GFW_ERR_HIP);
    if (stabs) HIP_TRY(sb.free_again(c->stream), GFW_ERR_HIP);
    for (int i = 0; i < count; ++i) out_ptrs[i] = (float *)buf.ptr + table_floats * i;
    if (c->synchronous) HIP_TRY(hipStreamSynchronize(c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
int gfw_build_matrices_batch(gfw_ctx *c, const gfw_frame_timing *t, int count, float **out_ptrs) {
    return gfw_build_matrices_batch_stab(c, t, nullptr, count, out_ptrs);
}
}
