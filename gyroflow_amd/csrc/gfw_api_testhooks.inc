// gfw_api_testhooks.inc — part of gfw_api.hip (textually included): the entry points of include/gfwarp_testing.h (device math probes, the host-side build check of
// the specialisation path, the shipped-cache key, gfw_checksum64 / gfw_set_frame_checksums, gfw_pack_matrices).  Split out of gfw_api.hip in round 6.

// ------------------------------------------------------------------------------------------------ test hooks
extern "C" {
int gfw_debug_math(int op, const float *a, const float *b, float *out, size_t n) {
    if (!a || !out || n == 0) { set_error("null/empty arrays"); return GFW_ERR_INVALID_ARGUMENT; }
    if (device_count() == 0) { set_error("no HIP device visible"); return GFW_ERR_NO_DEVICE; }
    HIP_TRY(hipSetDevice(g_current_device), GFW_ERR_HIP);
    DevBuf da, db, dout;                                     // (released on every path)
    HIP_TRY(da.ensure(n * sizeof(float)), GFW_ERR_HIP);
    HIP_TRY(dout.ensure(n * sizeof(float)), GFW_ERR_HIP);
    if (b) HIP_TRY(db.ensure(n * sizeof(float)), GFW_ERR_HIP);
    HIP_TRY(hipMemcpy(da.ptr, a, n * sizeof(float), hipMemcpyHostToDevice), GFW_ERR_HIP);
    if (b) HIP_TRY(hipMemcpy(db.ptr, b, n * sizeof(float), hipMemcpyHostToDevice), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_debug_math(op, (const float *)da.ptr, (const float *)db.ptr, (float *)dout.ptr, n, nullptr), GFW_ERR_HIP);
    HIP_TRY(hipMemcpy(out, dout.ptr, n * sizeof(float), hipMemcpyDeviceToHost), GFW_ERR_HIP);
    return GFW_OK;
}
long long gfw_debug_selftest(int test, unsigned long long n, unsigned long long seed) {
    if (device_count() == 0) { set_error("no HIP device visible"); return GFW_ERR_NO_DEVICE; }
    HIP_TRY(hipSetDevice(g_current_device), GFW_ERR_HIP);
    if (test == 2 && n == 0) n = 1ull << 31;
    DevBuf dbad;
    unsigned long long bad = 0;
    HIP_TRY(dbad.ensure(sizeof(bad)), GFW_ERR_HIP);
    HIP_TRY(hipMemset(dbad.ptr, 0, sizeof(bad)), GFW_ERR_HIP);
    HIP_TRY(gfw_launch_debug_selftest(test, n, seed, (unsigned long long *)dbad.ptr, nullptr), GFW_ERR_HIP);
    HIP_TRY(hipMemcpy(&bad, dbad.ptr, sizeof(bad), hipMemcpyDeviceToHost), GFW_ERR_HIP);
    return (long long)bad;
}
}

// Host-side build check of the run-time specialisation path (no device involved): compiles the embedded kernel source for `arch`
// with the given ';'-separated -D definitions and bake header; returns the code object's size (optionally written to `out_path`).
extern "C" long gfw_debug_jit_compile(const char *arch, const char *defines, const char *bake_header_text, const char *out_path, char *log, size_t cap) {
    if (!arch || !defines || !bake_header_text) return GFW_ERR_INVALID_ARGUMENT;
    std::vector<std::string> defs;
    split_defs(defines, defs);
    std::string lg;
    std::vector<char> code;
    const long n = gfw_jit_compile_only(arch, defs, bake_header_text, lg, &code);
    if (log && cap) snprintf(log, cap, "%s", lg.c_str());
    if (n > 0 && out_path && *out_path && !gfw_jit_write_code_object(out_path, code)) return GFW_ERR_UNKNOWN;
    return n;
}

// The host side of a radial model's first-pass certificate without a device (tests/test_emu_pass1_audit.py feeds the interpreted kernel with it): the table of
// GFW_P1_TABLE_N + 1 float pairs over r in [0, r_max] and {r_max, Tmax, T1, T2, e_table, nu2, d_min} (gfw_api_certificate.inc: p1_prepare_radial_gopro).
// Returns 1 when a certificate exists for these coefficients and this range, 0 when the host declines, a negative GFW_ERR_* on bad arguments.
extern "C" int gfw_debug_p1_radial(const gfw_kernel_params *params, int distortion_model, double r_max, float *table, double *out7) {
    if (!params || !out7 || !p1_model_radial(distortion_model)) { set_error("gfw_debug_p1_radial: model %d has no radial certificate", distortion_model); return GFW_ERR_INVALID_ARGUMENT; }
    P1Radial R; std::vector<float2> tab;
    if (!p1_prepare_radial(distortion_model, *params, r_max, R, table ? &tab : nullptr)) return 0;
    if (table) memcpy(table, tab.data(), tab.size() * sizeof(float2));
    out7[0] = R.r_max; out7[1] = R.Tmax; out7[2] = R.T1; out7[3] = R.T2; out7[4] = R.etab; out7[5] = R.nu2; out7[6] = R.dmin;
    return 1;
}
extern "C" int gfw_debug_source_id(char *out, size_t cap) {
    if (!out || cap == 0) return GFW_ERR_INVALID_ARGUMENT;
    const std::string id = gfw_jit_source_id();
    snprintf(out, cap, "%s", id.c_str());
    return (int)id.size();
}

static int jit_key_out(const char *arch, const std::vector<std::string> &defs, const std::string &header, char *defs_out, size_t defs_cap, char *header_out, size_t header_cap,
                       char *name_out, size_t name_cap) {
    std::string d;
    for (const std::string &x : defs) { if (!d.empty()) d += ";"; d += x; }
    const std::string name = gfw_jit_cache_name(arch, defs, header);
    if (!defs_out || !header_out || !name_out || d.size() + 1 > defs_cap || header.size() + 1 > header_cap || name.size() + 1 > name_cap) {
        set_error("output buffers too small"); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    memcpy(defs_out, d.c_str(), d.size() + 1); memcpy(header_out, header.c_str(), header.size() + 1); memcpy(name_out, name.c_str(), name.size() + 1);
    return GFW_OK;
}

// What run_planes would derive for frame 0 of the n_frames x F.nplanes planes in F.planes / F.params, each validated first, on a dry context: nothing touches a device
static int dry_fused_args(gfw_ctx &c, int n_frames, const FrameIn &F, ClipBatch *batch, GfwYuvArgs &Y, FusedShape &S) {
    { const int rc = check_pixel_types(F.nplanes, F.pixel_types); if (rc != GFW_OK) return rc; }
    for (int j = 0; j < n_frames * F.nplanes; ++j) { const int rc = validate_plane(&F.planes[j], &F.params[j], F.pixel_types[j % F.nplanes]); if (rc != GFW_OK) return rc; }
    c.dry = true;
    GfwPlane launches[4];
    memset(launches, 0, sizeof(launches));
    for (int i = 0; i < F.nplanes; ++i) { launches[i].src = (const uint8_t *)F.planes[i].input.data; launches[i].dst = (uint8_t *)F.planes[i].output.data; }
    bool served = false;
    { const int rc = build_yuv_args(&c, F, launches, batch, Y, S, served); if (rc != GFW_OK) return rc; }
    if (!served) { set_error("not a frame the fused kernel serves"); return GFW_ERR_UNSUPPORTED_BUFFER; }
    fill_common(&c, &F.params[0], nullptr, nullptr, 0, Y.common);
    return GFW_OK;
}

// Build-time helper of the shipped kernel cache (tools/build_jit_cache.py; no device involved): what the library WOULD specialise a frame of these planes to —
// the ';'-separated definition list, the bake header and the cache file name of the kernel (gfw_jit.hip) — exactly as run_planes / jit_for derive them on a
// device, with `matrices_on_device` as the context option would be set (2: device-resident tables, the first pass's table range from the intrinsics).
extern "C" int gfw_debug_jit_key(int nplanes, const gfw_buffers *planes, const gfw_kernel_params *params, const int *pixel_types, int distortion_model, int digital_lens,
                                 const float *h_matrices, int matrix_count, int matrices_on_device, const char *arch,
                                 char *defs_out, size_t defs_cap, char *header_out, size_t header_cap, char *name_out, size_t name_cap) {
    if (!planes || !params || !pixel_types || !arch || nplanes < 1 || nplanes > 4) { set_error("bad arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    gfw_ctx c;
    c.model = distortion_model; c.digital = digital_lens; c.matrices_on_device = matrices_on_device; c.arch = arch;
    GfwYuvArgs Y; FusedShape S;
    { const int rc = dry_fused_args(c, 1, FrameIn{nplanes, planes, params, pixel_types, h_matrices, matrix_count, nullptr, 0}, nullptr, Y, S); if (rc != GFW_OK) return rc; }
    return jit_key_out(arch, jit_build_defs(Y, S, CLIP_SHARED, false, nullptr), bake_header(Y, S, CLIP_SHARED), defs_out, defs_cap, header_out, header_cap, name_out, name_cap);
}

// The same for the first launch of a gfw_undistort_clip_params call (the per-frame flavour): `planes` / `params` hold n_frames x nplanes entries as that call takes
// them, so that the first pass's table is sized for the call's own envelope of fov and zoom centre; `host_matrices[f]` is frame f's rows[14] table (only frame 0's
// is read, and only with matrices_on_device = 0).  `audit`: the key under GFW_OPT_KERNEL_VARIANT 3 (the audit build).  Returns 1 (outputs untouched) when that launch
// would not be a specialised build at all (an audit of a frame without a certified first pass takes the ahead-of-time audit instantiations).
extern "C" int gfw_debug_jit_key_clip_params(int n_frames, int nplanes, const gfw_buffers *planes, const gfw_kernel_params *params, const int *pixel_types, int distortion_model,
                                             int digital_lens, const float *const *host_matrices, int matrix_count, int matrices_on_device, int audit, const char *arch,
                                             char *defs_out, size_t defs_cap, char *header_out, size_t header_cap, char *name_out, size_t name_cap) {
    if (!planes || !params || !pixel_types || !arch || n_frames < 1 || nplanes < 1 || nplanes > 4 || (!matrices_on_device && (!host_matrices || !host_matrices[0]))) {
        set_error("bad arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    gfw_ctx c;
    c.model = distortion_model; c.digital = digital_lens; c.matrices_on_device = matrices_on_device; c.arch = arch; c.kernel_variant = audit ? 3 : 0;
    ClipBatch batch(CLIP_PER_FRAME, n_frames, nplanes, params);
    GfwYuvArgs Y; FusedShape S;
    { const int rc = dry_fused_args(c, n_frames, FrameIn{nplanes, planes, params, pixel_types, matrices_on_device ? nullptr : host_matrices[0], matrix_count, nullptr, 0}, &batch, Y, S);
      if (rc != GFW_OK) return rc; }
    const bool audit_build = jit_audit_build(&c, Y, CLIP_PER_FRAME);
    if ((c.kernel_variant != 0 || Y.audit) && !audit_build) return 1;             // (jit_for: the ahead-of-time kernel)
    return jit_key_out(arch, jit_build_defs(Y, S, CLIP_PER_FRAME, audit_build, nullptr), bake_header(Y, S, CLIP_PER_FRAME), defs_out, defs_cap, header_out, header_cap, name_out, name_cap);
}

// The same for the first launch of a gfw_undistort_clip_lens call (the moving-lens flavour): `mesh_lens` as that call takes it (NULL: no frame has a mesh; the
// meshes' contents do not enter the key, only whether frame 0 has one).  A call in which no lens field moves and no frame has a mesh answers as
// gfw_debug_jit_key_clip_params does (audit 0).  Returns 1 (outputs untouched) where an ahead-of-time kernel would run.
extern "C" int gfw_debug_jit_key_clip_lens(int n_frames, int nplanes, const gfw_buffers *planes, const gfw_kernel_params *params, const int *pixel_types, int distortion_model,
                                           int digital_lens, const float *const *host_matrices, int matrix_count, int matrices_on_device, const size_t *mesh_lens, const char *arch,
                                           char *defs_out, size_t defs_cap, char *header_out, size_t header_cap, char *name_out, size_t name_cap) {
    if (!planes || !params || !pixel_types || !arch || n_frames < 1 || nplanes < 1 || nplanes > 4 || (!matrices_on_device && (!host_matrices || !host_matrices[0]))) {
        set_error("bad arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    if (!lens_moves(n_frames, nplanes, params, [&](int f) { return mesh_lens && mesh_lens[f]; })) return gfw_debug_jit_key_clip_params(n_frames, nplanes, planes, params, pixel_types, distortion_model, digital_lens, host_matrices, matrix_count, matrices_on_device, 0, arch,
                                                     defs_out, defs_cap, header_out, header_cap, name_out, name_cap);
    const size_t ml0 = mesh_lens ? mesh_lens[0] : 0;
    if (ml0 > GFW_MESH_MAX) { set_error("frame 0: mesh of %zu values", ml0); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    gfw_ctx c;
    c.model = distortion_model; c.digital = digital_lens; c.matrices_on_device = matrices_on_device; c.arch = arch;
    ClipBatch batch(CLIP_MOVING_LENS, n_frames, nplanes, params);
    GfwYuvArgs Y; FusedShape S;
    static const float no_mesh[GFW_MESH_MAX] = {};      // (fused_eligible asks only whether a mesh is there)
    { const int rc = dry_fused_args(c, n_frames, FrameIn{nplanes, planes, params, pixel_types, matrices_on_device ? nullptr : host_matrices[0], matrix_count, ml0 ? no_mesh : nullptr, ml0}, &batch, Y, S);
      if (rc != GFW_OK) return rc; }
    return jit_key_out(arch, jit_build_defs(Y, S, CLIP_MOVING_LENS, false, nullptr), bake_header(Y, S, CLIP_MOVING_LENS), defs_out, defs_cap, header_out, header_cap, name_out, name_cap);
}

extern "C" int gfw_checksum64(gfw_ctx *c, const void *d_buf, size_t bytes, unsigned long long *d_out) {
    if (!c || !d_buf || !d_out || (bytes & 7) || ((uintptr_t)d_buf & 15)) { set_error("bad checksum arguments"); return GFW_ERR_INVALID_ARGUMENT; }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }

    HIP_TRY(gfw_launch_checksum64(d_buf, bytes, d_out, c->stream), GFW_ERR_HIP);
    return GFW_OK;
}

extern "C" int gfw_set_frame_checksums(gfw_ctx *c, unsigned long long *d_sums, size_t count) {
    if (!c) { set_error("null context"); return GFW_ERR_INVALID_ARGUMENT; }
    { const int frc_ = flush_if_pending(c); if (frc_ != GFW_OK) return frc_; }          // frames being held were submitted under the previous setting
    c->sums = (d_sums && count) ? d_sums : nullptr; c->sum_n = c->sums ? count : 0; c->sum_k = 0;
    return GFW_OK;
}

extern "C" int gfw_pack_matrices(const float *rows14, int count, float *rows16) {
    if (!rows14 || !rows16 || count < 0) { set_error("null arrays"); return GFW_ERR_INVALID_ARGUMENT; }
    for (int r = 0; r < count; ++r) pack_row(rows14 + (size_t)r * 14, rows16 + (size_t)r * GFW_MAT_STRIDE);
    return GFW_OK;
}
extern "C" long long gfw_debug_paired_launches(gfw_ctx *c) { return c ? c->paired_launches : -1; }
extern "C" int gfw_debug_frames_per_launch(unsigned long long bytes_per_frame, unsigned long long budget_bytes, int frames_in_call) {
    return clip_frames_per_launch((size_t)bytes_per_frame, budget_bytes ? (size_t)budget_bytes : clip_launch_bytes(), frames_in_call);
}
