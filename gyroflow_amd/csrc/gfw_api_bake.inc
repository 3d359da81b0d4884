// gfw_api_bake.inc — run-time specialisation, host side: the bake header, the definition list, the per-clip kernel lookup (included by gfw_api.hip: one translation unit)
// ---- run-time specialisation (gfw_jit.hip) ----------------------------------------------------------------------------------------
// The bake header: every clip-invariant field of the fused kernel's argument block as a literal, GFW_BK_<field> (floats by bit
// pattern; gfw_frame.hip reads them through AF()).  What stays
// an argument: plane pointers and lengths, the matrix table, the first-pass table and its three range constants (the table may be
// rebuilt mid-clip), the grid.  Two frames with the same header run the same specialised kernel.
static void bake_f(std::string &o, const char *name, float v) {
    uint32_t u; memcpy(&u, &v, 4);
    char b[128]; snprintf(b, sizeof(b), "#define GFW_BK_%s __builtin_bit_cast(float, 0x%08xu)\n", name, u); o += b;
}
static void split_defs(const char *text, std::vector<std::string> &defs) {             // a ';'-separated definition list, appended
    std::string cur;
    for (const char *p = text; ; ++p) { if (*p == ';' || *p == 0) { if (!cur.empty()) defs.push_back(cur); cur.clear(); if (!*p) break; } else cur += *p; }
}
static void bake_i(std::string &o, const char *name, long long v) { char b[128]; snprintf(b, sizeof(b), "#define GFW_BK_%s (%lld)\n", name, v); o += b; }
// Luma block rows per lane of a SPECIALISED kernel (its tile = 64 DW x 4 RB DH luma pixels): the ahead-of-time kernels' by default; GFW_JIT_RB_FAST in the
// environment scans it for the certified first pass (whose cost per pixel — the lattice's nodes, the queue's resolution — is per tile).
static int jit_rows(bool fast1) {
    static const int env = [] { const char *e = getenv("GFW_JIT_RB_FAST"); const int v = e ? atoi(e) : 0; return (v >= 1 && v * 4 <= 64) ? v : 0; }();
    return (fast1 && env > 0) ? env : gfw_yuv_rows_per_lane(fast1, 0);
}
// CLIP_PER_FRAME (GFW_JIT_PERFRAME, gfw_undistort_clip_params): translation2d and FILL_WITH_BACKGROUND are not literals there (the kernel reads them from each
// frame's slot), so they are left out: a use that slipped past the flavour would not compile.  CLIP_MOVING_LENS (gfw_undistort_clip_lens): f, c, k and r_limit_sq
// come from each frame's lens slot and are left out in the same way (p1_f / p1_c, the first pass's copies of f and c, are zero: the flavour takes the exact first
// pass, build_yuv_args sets no certified one up).
static std::string bake_header(const GfwYuvArgs &Y_in, const FusedShape &S, ClipFlavour flavour) {
    const bool in_slot = flavour >= CLIP_PER_FRAME, in_lens_slot = flavour >= CLIP_MOVING_LENS;      // where the kernel reads the field from
    GfwYuvArgs Y = Y_in;
    Y.tiles_y = tiles_y_of(Y, jit_rows(S.fast1 != 0));                                       // (the launch's own tiling: the argument block carries the ahead-of-time kernels')
    std::string o;
    o.reserve(4096);
    bake_i(o, "nplanes", Y.nplanes); bake_i(o, "width", Y.width); bake_i(o, "height", Y.height); bake_i(o, "out_w", Y.out_w); bake_i(o, "out_h", Y.out_h);
    bake_i(o, "cw", Y.cw); bake_i(o, "ch", Y.ch); bake_i(o, "tiles_x", Y.tiles_x); bake_i(o, "tiles_y", Y.tiles_y); bake_i(o, "matrix_count", Y.matrix_count);
    bake_i(o, "hrs", Y.hrs); bake_i(o, "model", Y.model); bake_i(o, "k_all_zero", Y.k_all_zero);
    bake_i(o, "background_mode", Y.background_mode); bake_i(o, "extras", Y.extras); bake_i(o, "ablate", 0);
    bake_i(o, "digital", (Y.extras & 2) ? Y.common.digital : 0);
    if (!in_slot) bake_i(o, "fill_bg", Y.fill_bg);
    bake_i(o, "rot_on", Y.rot_on); bake_i(o, "fix_range", Y.fix_range); bake_i(o, "checksum", Y.checksum);
    bake_i(o, "hstretch_div", Y.hstretch_div); bake_i(o, "vstretch_div", Y.vstretch_div); bake_f(o, "hstretch", Y.hstretch); bake_f(o, "vstretch", Y.vstretch);
    // (an audit build — GFW_OPT_KERNEL_VARIANT 3 / 4 on a clip whose certified first pass lives in specialised builds only, the radial models' — reads the counters' address from the arguments)
    o += Y.audit ? "#define GFW_BK_audit (A.audit)\n" : "#define GFW_BK_audit ((unsigned long long *)nullptr)\n";
    { char b[64]; snprintf(b, sizeof(b), "#define GFW_P1_RFORM (%d)\n", Y.p1_rform ? 1 : 0); o += b; }
    char nm[48];
    for (int i = 0; i < 2; ++i) { if (!in_lens_slot) { snprintf(nm, sizeof(nm), "f_%d", i); bake_f(o, nm, Y.f[i]); snprintf(nm, sizeof(nm), "c_%d", i); bake_f(o, nm, Y.c[i]); }
                                  if (!in_slot) { snprintf(nm, sizeof(nm), "t2_%d", i); bake_f(o, nm, Y.t2[i]); } }
    if (!in_lens_slot) {
        for (int i = 0; i < 4; ++i) { snprintf(nm, sizeof(nm), "k_%d", i); bake_f(o, nm, Y.k[i]); }
        bake_f(o, "r_limit_sq", Y.r_limit_sq);
    }
    const GfwMapConst *maps[4] = {&Y.map_lx, &Y.map_ly, &Y.map_cx, &Y.map_cy};
    const char *mn[4] = {"map_lx", "map_ly", "map_cx", "map_cy"};
    for (int i = 0; i < 4; ++i) {
        snprintf(nm, sizeof(nm), "%s_mul", mn[i]); bake_f(o, nm, maps[i]->mul);
        snprintf(nm, sizeof(nm), "%s_den", mn[i]); bake_f(o, nm, maps[i]->den);
        snprintf(nm, sizeof(nm), "%s_rcp", mn[i]); bake_f(o, nm, maps[i]->rcp);
    }
    bake_f(o, "p1_f", Y.p1_f); bake_f(o, "p1_c", Y.p1_c);
    for (int i = 0; i < 4; ++i) {
        const GfwYuvPlane &P = Y.pl[i];
        snprintf(nm, sizeof(nm), "pl%d_src_stride", i); bake_i(o, nm, P.src_stride);
        snprintf(nm, sizeof(nm), "pl%d_dst_stride", i); bake_i(o, nm, P.dst_stride);
        snprintf(nm, sizeof(nm), "pl%d_w", i); bake_i(o, nm, P.w);
        snprintf(nm, sizeof(nm), "pl%d_h", i); bake_i(o, nm, P.h);
        for (int ch = 0; ch < 4; ++ch) { snprintf(nm, sizeof(nm), "pl%d_bg_%d", i, ch); bake_f(o, nm, P.bg[ch]); }
        snprintf(nm, sizeof(nm), "pl%d_limit", i); bake_f(o, nm, P.limit);
        snprintf(nm, sizeof(nm), "pl%d_fix", i); bake_i(o, nm, P.fix);
        snprintf(nm, sizeof(nm), "pl%d_org_x", i); bake_f(o, nm, P.org_x); snprintf(nm, sizeof(nm), "pl%d_org_y", i); bake_f(o, nm, P.org_y);
        snprintf(nm, sizeof(nm), "pl%d_ox32", i); bake_i(o, nm, P.ox32); snprintf(nm, sizeof(nm), "pl%d_oy32", i); bake_i(o, nm, P.oy32);
    }
    return o;
}
// Waves per SIMD the specialised instantiation is budgeted for.  Measured on MI355X (us per frame, priority step of its time; gpurun_out/r03b-m,
// profiles/r03_ab_waves_priority.txt): C2 bilinear 6 -> 65.4, 7 -> 57.0-59.3, 8 -> 55.0; NV12 64.6 -> 60.5, P010 71.4 -> 67.8, planar f32 97.7 -> 91.5,
// Lanczos4 180.5 -> 173.6, bicubic 96.3 -> 95.4, fisheye + SuperView 117.3 -> 103.7 at 7 -> 8.  Eight waves lose where a wave's life is short or
// its registers are many: one matrix per frame (C1 1080p: 9.30 at 7, 10.2 at 8) and packed RGBA planes (C4: 73.0 at 7, 74.7 at 8) stay at seven.
// The generic-model body keeps the rule — the lens-correction blend too, although it spills a few dwords at eight waves (GoPro lens, blend 0.5:
// 141.5 us at 6 waves, 139.2 at 7, 134.4 at 8; fisheye + blend 140.5 / 137.4 / 135.9) — except with background mode 3 or the Sony mesh (two
// samples per pixel, f64 splines: up to 80 registers), which get six.
static int jit_waves(const FusedShape &S, int matrix_count, int jit_model, int extras, int checksum = 0) {
    const int n0 = S.n0, taps = S.taps, bps = S.kind;
    static const int forced = getenv("GFW_JIT_WAVES") ? atoi(getenv("GFW_JIT_WAVES")) : 0;      // experiments
    if (forced >= 1 && forced <= 8) return forced;
    // The checksum build (gfw_set_frame_checksums) keeps three more registers alive through the tile walk; at eight waves (64 registers) four dwords go to scratch, and
    // every build of this kernel with a private segment measured 4-10 % slower than its scratch-free twin (all waves resident, same instruction count: not occupancy —
    // profiles/r05_c5_checksum.txt): C5 46.4 us per frame at eight waves, 44.6 at seven — no scratch
    if (checksum) { const int w = jit_waves(S, matrix_count, jit_model, extras, 0); return w == 8 ? 7 : w; }
    if (jit_model < 0 && (extras & (16 | 32))) return 6;
    // bicubic / Lanczos4 on single-channel integer planes: registers for the tap rows in flight are worth more than the seventh and eighth wave
    // (gfw_frame.hip GFW_TAP_ROW_UNROLL; profiles/r04_ab_lut_rows.txt).  Round 5: C2's bicubic (16-bit, full-height chroma) too — with the group-first row fetch the
    // six-wave build is the same 64.5 us from the ROCm 7.0 hiprtc torch brings and from the system's 7.2 (it had been 64 against 78), against 68.3 at eight waves
    // (profiles/r05_first_call.txt).
    if (n0 == 1 && bps <= 2 && taps == 4) return 6;
    if (n0 == 1 && bps <= 2 && taps == 8) return bps == 1 ? 5 : 6;
    return (n0 == 1 && matrix_count > 1) ? 8 : 7;
}
static int jit_model_of(const GfwYuvArgs &Y) {
    return (Y.model == GFW_MODEL_OPENCV_FISHEYE && (Y.extras & ~2) == 0) ? GFW_MODEL_OPENCV_FISHEYE : ((Y.extras & (16 | 32)) ? -2 : -1);
}
// Whether an audit (GFW_OPT_KERNEL_VARIANT 3 / 4) takes a specialised audit build (GFW_JIT_AUDIT=1) rather than the ahead-of-time audit instantiations: where the
// first pass to be audited lives in specialised builds only — a table over r (the radial models), and every launch of the per-frame flavour, whose certificate
// half-width is each frame's own (its translation2d) and whose kernel no ahead-of-time instantiation is
static bool jit_audit_build(const gfw_ctx *c, const GfwYuvArgs &Y, ClipFlavour flavour) {
    return Y.audit && (Y.p1_rform || flavour != CLIP_SHARED) && (c->kernel_variant == 3 || c->kernel_variant == 4);
}
// The definition list of a specialised build (with the bake header: everything that names the kernel; also behind the gfw_debug_jit_key hooks); `waves_out`: the budget
static std::vector<std::string> jit_build_defs(const GfwYuvArgs &Y, const FusedShape &S, ClipFlavour flavour, bool audit_build, int *waves_out) {
    const int jit_model = jit_model_of(Y);
    int waves = jit_waves(S, Y.matrix_count, jit_model, Y.extras, Y.checksum);
    // (the per-frame flavour of the lens-correction body keeps one more value of the frame alive through the pixel loop: at eight waves 24 bytes went to scratch
    // on 4K NV12, so it gets seven — as the checksum build does; every other body keeps its constant build's waves: tests/test_kernel_resources_perframe.py)
    // (the moving-lens flavour keeps the per-frame flavour's budget: compiled beside flavour 1 with the exact first pass it shows no scratch where that has none —
    // 4K C2 53 registers against 54, the lens-correction body 72 / 72, the mesh body 80 / 80 with less scratch: tests/test_kernel_resources_perlens.py)
    if (flavour != CLIP_SHARED && (Y.extras & 8) && waves == 8) waves = 7;
    char b[64];
    std::vector<std::string> defs;
    snprintf(b, sizeof(b), "GFW_FRAME_KIND=%d", S.kind); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_FRAME_TAPS=%d", S.taps); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_WAVES=%d", waves); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_MODEL=%d", jit_model); defs.push_back(b);
    defs.push_back(S.kind == 1 ? "GFW_JIT_T=uint8_t" : S.kind == 2 ? "GFW_JIT_T=uint16_t" : S.kind == 3 ? "GFW_JIT_T=_Float16" : "GFW_JIT_T=float");
    snprintf(b, sizeof(b), "GFW_JIT_N0=%d", S.n0); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_DW=%d", S.dw); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_DH=%d", S.dh); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_IL=%d", S.interleaved ? 1 : 0); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_RB=%d", jit_rows(S.fast1 != 0)); defs.push_back(b);
    snprintf(b, sizeof(b), "GFW_JIT_FAST1=%d", S.fast1 ? 1 : 0); defs.push_back(b);
    if (flavour != CLIP_SHARED) { snprintf(b, sizeof(b), "GFW_JIT_PERFRAME=%d", (int)flavour); defs.push_back(b); }      // (absent for CLIP_SHARED: its definition lists — the cache names — are what they were before the flavours)
    if (const char *extra = getenv("GFW_JIT_DEFS")) split_defs(extra, defs);             // experiments: further ';'-separated definitions for the build
    if (audit_build) defs.push_back("GFW_JIT_AUDIT=1");
    if (waves_out) *waves_out = waves;
    return defs;
}
// The specialised kernel for this frame's arguments, or nullptr (not eligible / not wanted / not ready / failed): the caller then
// launches the ahead-of-time kernel.  `flavour`: of the launch the frame is for — the key blanks the fields the frames carry in that flavour's slots as well
// (clip_blank_slots), so that one kernel serves the clip and the kJitAfter count runs on under a moving zoom centre (CLIP_PER_FRAME) or a moving lens
// (CLIP_MOVING_LENS).  (k_all_zero and every `extras` bit stay in the key: the kernel is compiled for them.)
static hipFunction_t jit_for(gfw_ctx *c, const GfwYuvArgs &Y, const FusedShape &S, ClipFlavour flavour, int *grid) {
    // every frame the fused kernel serves can be specialised: the fisheye model alone or under a digital lens (extras 0 / 2) takes the lean
    // projection (MODEL = 1); everything else the generic-model body with the lens model, the digital lens and the feature bits as literals
    // (MODEL = -1, or -2 with background mode 3 / the Sony mesh) — the run-time switch over 14 lens models folds to the one in use
    // (kernel variants and the audit take the ahead-of-time instantiations — except the audit of a table over r and of a per-frame launch: jit_audit_build)
    const bool audit_build = jit_audit_build(c, Y, flavour);
    if (c->jit_mode == 0 || ((c->kernel_variant != 0 || Y.audit) && !audit_build) || Y.ablate) return nullptr;
    // the same clip as the previous frame?  Compared on the argument block itself with its per-frame fields blanked (the header text and the
    // cache lookup cost ~15 us of host time, a frame's worth of validation): header, key and function are rebuilt only when it changes
    GfwYuvArgs K = Y;
    clip_blank_slots(K, flavour);
    for (int i = 0; i < 4; ++i) { K.pl[i].src = nullptr; K.pl[i].dst = nullptr; K.pl[i].src_len = 0; K.pl[i].dst_len = 0; }
    K.matrices = nullptr; K.p1_table = nullptr; K.p1_rho_max = 0.0f; K.p1_rho_scale = 0.0f; K.p1_eps = 0.0f; K.p1_ew = 0.0f; K.p1_em = 0.0f; K.p1_kmax = 0.0f; K.audit = Y.audit ? (unsigned long long *)1 : nullptr; K.ck_part = nullptr; K.grid_limit = 0;
    memset(K.p1_lat, 0, sizeof(K.p1_lat));
    memset(&K.kp, 0, sizeof(K.kp));
    { const int dig = K.common.digital; memset(&K.common, 0, sizeof(K.common)); K.common.digital = dig; }
    const JitKeyMisc misc = {S, c->tune_grid, flavour};
    const bool same = c->jit_key_valid && memcmp(&K, &c->jit_key, sizeof(K)) == 0 && memcmp(&misc, &c->jit_key_misc, sizeof(misc)) == 0;
    if (same) {
        if (c->jit_seen < (1 << 30)) ++c->jit_seen;
        if (c->jit_fn) { *grid = c->jit_grid; return c->jit_fn; }                        // ready and loaded: nothing else to do
        if (c->jit_dead) return nullptr;                                                 // decided: ahead of time for the rest of the clip, no lookup per frame
    } else {
        jit_reset(c);
        c->jit_key = K; c->jit_key_misc = misc; c->jit_key_valid = true;
        c->jit_header = bake_header(Y, S, flavour); c->jit_seen = 1;
    }
    if (c->jit_mode == 1 && c->jit_seen < gfw_ctx::kJitAfter && !audit_build) return nullptr;          // one or two frames are not a clip
    int waves = 0;
    const std::vector<std::string> defs = jit_build_defs(Y, S, flavour, audit_build, &waves);
    hipFunction_t fn = gfw_jit_get(c->device, c->arch, defs, c->jit_header, c->jit_mode == 2 || audit_build, &c->jit_info);
    if (!fn) { c->jit_dead = c->jit_info.state == GFW_JIT_FAILED || c->jit_info.state == GFW_JIT_UNAVAILABLE; return nullptr; }
    int g = c->tune_grid > 0 ? c->tune_grid : c->num_cus * waves;
    const int per_xcd = (Y.tiles_x * tiles_y_of(Y, jit_rows(S.fast1 != 0)) + 7) >> 3;
    if (g > per_xcd * 8) g = per_xcd * 8;
    *grid = (g + 7) & ~7;
    c->jit_fn = fn; c->jit_grid = *grid;
    return fn;
}

