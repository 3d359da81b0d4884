// gfw_api_eligibility.inc — which frames the fused kernel serves, and its argument block (included by gfw_api.hip: one translation unit)
// Decide whether the frame qualifies for the fused YUV kernel and, if so, build its argument block.
// Anything not proven here runs through the generic per-plane kernel (same results, slower).
// fused_eligible answers from the frame's description alone (no device work): true with Y and S filled but for the first pass and the tiling.
static bool fused_eligible(const gfw_ctx *c, const FrameIn &F, const GfwPlane *launches, const float *h_matrices, GfwYuvArgs &Y, FusedShape &S) {
    const int nplanes = F.nplanes, matrix_count = F.matrix_count, *pixel_types = F.pixel_types; const size_t mesh_len = F.mesh_len;
    const gfw_buffers *planes = F.planes; const gfw_kernel_params *params = F.params;
    S = FusedShape();
    int &bytes_per_sample = S.kind, &n0 = S.n0, &dw = S.dw, &dh = S.dh, &interleaved = S.interleaved;
    if (c->kernel_variant == 1) return false;                       // forced generic (tests / A-B benchmarking)
    if (nplanes < 1 || nplanes > 4) return false;
    const gfw_kernel_params &p0 = params[0];
    const int t0 = pixel_types[0];
    // a plane's effective size on either side: its rect's (validated per plane below)
    auto in_w = [&](int i) { return params[i].source_rect[2]; };  auto in_h = [&](int i) { return params[i].source_rect[3]; };
    auto out_w = [&](int i) { return params[i].output_rect[2]; }; auto out_h = [&](int i) { return params[i].output_rect[3]; };
    // plane 0: sample kind (1 = u8, 2 = u16, 4 = f32) and channel count; RGBAf16 / UV-as-plane-0 stay on the generic kernel
    switch (t0) {
    case GFW_PIX_LUMA8:  bytes_per_sample = 1; n0 = 1; break;
    case GFW_PIX_LUMA16: bytes_per_sample = 2; n0 = 1; break;
    case GFW_PIX_RGB8:   bytes_per_sample = 1; n0 = 3; break;
    case GFW_PIX_RGBA8: case GFW_PIX_BGRA8: bytes_per_sample = 1; n0 = 4; break;
    case GFW_PIX_RGB16:  bytes_per_sample = 2; n0 = 3; break;
    case GFW_PIX_RGBA16: case GFW_PIX_AYUV16: bytes_per_sample = 2; n0 = 4; break;
    case GFW_PIX_RGBAF:  bytes_per_sample = 4; n0 = 4; break;
    case GFW_PIX_RGBAF16: bytes_per_sample = 3; n0 = 4; break;       // (sample KIND 3: two-byte float samples — the kernels' _Float16 instantiations; round 5)
    case GFW_PIX_R32F:   bytes_per_sample = 4; n0 = 1; break;
    default: return false;
    }
    if (n0 > 1 && nplanes != 1) return false;
    interleaved = 0;
    if (nplanes >= 2) {
        const int t1 = pixel_types[1];
        if (bytes_per_sample != 4 && t1 == (bytes_per_sample == 1 ? GFW_PIX_UV8 : GFW_PIX_UV16)) { if (nplanes != 2) return false; interleaved = 1; }
        else { for (int i = 1; i < nplanes; ++i) if (pixel_types[i] != t0) return false; }
    }
    int extras = 0;
    if (mesh_len != 0) extras |= 32;
    if (c->digital != GFW_MODEL_NONE && (p0.flags & GFW_FLAG_HAS_DIGITAL_LENS)) extras |= 2;
    if (c->model < GFW_MODEL_OPENCV_FISHEYE || c->model > GFW_MODEL_GOPRO) return false;
    // plane-invariant parameters must really be invariant, and inside the fused kernel's feature set
    for (int i = 0; i < nplanes; ++i) {
        const gfw_kernel_params &p = params[i];
        if ((p.interpolation != 2 && p.interpolation != 4 && p.interpolation != 8) || p.interpolation != p0.interpolation) return false;
        if (p.background_mode < 0 || p.background_mode > 3 || p.background_mode != p0.background_mode || p.input_rotation != p0.input_rotation || !(p.input_rotation == p.input_rotation)) return false;
        if (p.background_mode == 3) {
            if (p.background_margin != p0.background_margin || p.background_margin_feather != p0.background_margin_feather) return false;
            extras |= 16;                                                        // two samples + blend (:576-613), generic-model instantiation
        }
        if (!(p.lens_correction_amount == p.lens_correction_amount) || p.lens_correction_amount != p0.lens_correction_amount) return false;
        if (p.lens_correction_amount < 1.0f) extras |= 8;                        // the blend of :429-460 (generic-model instantiation)
        if (!(p.light_refraction_coefficient == p.light_refraction_coefficient) || p.light_refraction_coefficient != p0.light_refraction_coefficient) return false;
        if (p.light_refraction_coefficient != 1.0f && p.light_refraction_coefficient > 0.0f) extras |= 4;
        if ((p.flags ^ p0.flags) & GFW_FLAG_HAS_DIGITAL_LENS) return false;
        if (mesh_len != 0 && ((p.flags ^ p0.flags) & 128)) return false;          // the mesh terms read flag 128 (vertically flipped frame buffer)
        if (memcmp(p.digital_lens_params, p0.digital_lens_params, sizeof(p.digital_lens_params))) return false;
        if ((p.flags ^ p0.flags) & GFW_FLAG_FIX_COLOR_RANGE) return false;         // (FIX_COLOR_RANGE — the render loop raises it for macOS VideoToolbox, rendering/mod.rs:507-509 — on every plane or none)
        if ((p.flags & GFW_FLAG_FIX_COLOR_RANGE) && p.plane_index != i) return false; // (the scale follows plane_index == 0, cpu_undistort.rs:620: the planes in their own order)
        if ((p.flags ^ p0.flags) & GFW_FLAG_FILL_WITH_BACKGROUND) return false;
        if (p.translation3d[0] != 0.0f || p.translation3d[1] != 0.0f || p.translation3d[2] != 0.0f) return false;
        if (p.width != p0.width || p.height != p0.height || p.output_width != p0.output_width || p.output_height != p0.output_height) return false;
        if (p.matrix_count != p0.matrix_count || ((p.flags ^ p0.flags) & GFW_FLAG_HORIZONTAL_RS)) return false;
        if (memcmp(p.f, p0.f, sizeof(p.f)) || memcmp(p.c, p0.c, sizeof(p.c)) || memcmp(p.k, p0.k, sizeof(p.k))) return false;
        if (memcmp(p.translation2d, p0.translation2d, sizeof(p.translation2d)) || p.r_limit != p0.r_limit || p.fov != p0.fov) return false;
        if (p.input_horizontal_stretch != p0.input_horizontal_stretch || p.input_vertical_stretch != p0.input_vertical_stretch) return false;
        // Rects (round 6): the plane occupies source_rect / output_rect of its buffer (mod.rs:209-224, 322-323: a BufferDescription's rect — set by hosts that hand
        // over a window of a larger surface — else the whole buffer).  The kernel works on the rect as if it were the plane: pointers rebased to the rect's first
        // pixel (below), sizes = the rect's; what does NOT rebase is the source coordinate's `+ source_rect origin` (cpu_undistort.rs:510-515), which rounds before
        // the 1/32-pixel binning: the kernel adds the origin as the reference does and takes 32 * origin off the bins (GfwYuvPlane.org_x / ox32).
        const gfw_buffers &b = planes[i];
        if (p.source_rect[0] < 0 || p.source_rect[1] < 0 || p.source_rect[2] <= 0 || p.source_rect[3] <= 0) return false;
        if (p.output_rect[0] < 0 || p.output_rect[1] < 0 || p.output_rect[2] <= 0 || p.output_rect[3] <= 0) return false;
        if ((int64_t)p.source_rect[0] + p.source_rect[2] > b.input.width || (int64_t)p.source_rect[1] + p.source_rect[3] > b.input.height) return false;
        if ((int64_t)p.output_rect[0] + p.output_rect[2] > b.output.width || (int64_t)p.output_rect[1] + p.output_rect[3] > b.output.height) return false;
        if (p.source_rect[0] > 32767 || p.source_rect[1] > 32767) return false;                  // (32 * origin as a 24-bit integer, the origin exact in f32)
        if (p.stride <= 0 || b.output.stride <= 0) return false;
        if ((int64_t)b.input.height * p.stride > (int64_t)b.input.len) return false;
        if ((int64_t)b.output.height * b.output.stride > (int64_t)b.output.len) return false;
        if ((int64_t)b.output.width * p.bytes_per_pixel > b.output.stride) return false;
        // rows of the buffer beyond the plane would be visited (and skipped) by the reference; require none carry pixels
        if ((bytes_per_sample == 2 || bytes_per_sample == 3) && ((p.stride | b.output.stride) & 1)) return false;
        if ((bytes_per_sample == 4) && ((p.stride | b.output.stride) & 3)) return false;
        if ((int64_t)b.input.height * p.stride >= (1ll << 31) || (int64_t)b.output.height * b.output.stride >= (1ll << 31)) return false;   // 32-bit offsets
        if (p.stride >= (1 << 23) || b.output.stride >= (1 << 23) || b.input.height >= (1 << 23) || b.output.height >= (1 << 23)) return false;   // 24-bit row-offset multiplies
    }
    // stretch divisions (cpu_undistort.rs:222-223): "skipped" (<= 0.001) and the identity x / 1 cost nothing; a real divisor (anamorphic lens profiles) is an
    // IEEE division at the end of the projection, served since round 4 (not together with the lens-correction blend, whose inverse the kernel does not stretch)
    if (!(p0.input_horizontal_stretch == p0.input_horizontal_stretch) || !(p0.input_vertical_stretch == p0.input_vertical_stretch)) return false;
    const bool hdiv = p0.input_horizontal_stretch > 0.001f && p0.input_horizontal_stretch != 1.0f, vdiv = p0.input_vertical_stretch > 0.001f && p0.input_vertical_stretch != 1.0f;
    if ((hdiv || vdiv) && ((extras & 8) || !std::isfinite(p0.input_horizontal_stretch) || !std::isfinite(p0.input_vertical_stretch))) return false;
    for (int i = 0; i < 12; ++i) { const float k = p0.k[i]; if (!(k == k) || fabsf(k) > 1024.0f) return false; }
    if (!std::isfinite(p0.f[0]) || !std::isfinite(p0.f[1]) || !std::isfinite(p0.c[0]) || !std::isfinite(p0.c[1])) return false;
    if (!(p0.translation2d[0] == p0.translation2d[0]) || !(p0.translation2d[1] == p0.translation2d[1])) return false;
    // luma plane is full resolution on both sides
    if (in_w(0) != p0.width || in_h(0) != p0.height) return false;
    if (out_w(0) != p0.output_width || out_h(0) != p0.output_height) return false;
    dw = 1; dh = 1;
    if (nplanes >= 2) {
        const int cw = out_w(1), ch = out_h(1);
        if (cw <= 0 || ch <= 0 || p0.output_width % cw || p0.output_height % ch) return false;
        dw = p0.output_width / cw; dh = p0.output_height / ch;
        if (!((dw == 1 && dh == 1) || (dw == 2 && dh == 1) || (dw == 2 && dh == 2))) return false;
        if (bytes_per_sample == 4 && !(dw == 1 && dh == 1)) return false;
        for (int i = 1; i < nplanes; ++i) {
            if (out_w(i) != cw || out_h(i) != ch) return false;
            if (in_w(i) * dw != p0.width || in_h(i) * dh != p0.height) return false;
            // (the chroma planes share one set of bins: one source origin)
            if (params[i].source_rect[0] != params[1].source_rect[0] || params[i].source_rect[1] != params[1].source_rect[1]) return false;
            // planar chroma planes share one set of offsets in the kernel
            if (params[i].stride != params[1].stride || planes[i].output.stride != planes[1].output.stride) return false;
        }
        // chroma site -> luma position identity: xc*ow exact and (xc*ow)/(ow/dw) = dw*xc   (util.rs:144-147)
        if (!int_products_exact(cw, p0.output_width) || !int_products_exact(ch, p0.output_height)) return false;
    }
    // luma output pixel -> output space identity: x*ow/ow = x
    if (!int_products_exact(p0.output_width, p0.output_width) || !int_products_exact(p0.output_height, p0.output_height)) return false;
    if (p0.output_width >= (1 << 23) || p0.output_height >= (1 << 23)) return false;
    if (p0.width > 65535 || p0.height > 65535) return false;                // the first pass keeps its row / column indices in 16 bits (s_rows)
    // IBIS/OIS terms (matrices[9..13]): host matrices are scanned, device matrices rely on the flag (get_kernel_flags sets
    // it whenever the clip has IBIS/OIS data, mod.rs:226-251); packed device rows carry cos/sin of the roll from
    // gfw_pack_matrices, raw device rows[14] get them from gfw_repack_matrices_kernel (the same libm routines, restated)
    if (h_matrices) {
        for (int r = 0; r < matrix_count && !(extras & 1); ++r) { const float *m = h_matrices + (size_t)r * 14;
            if (m[9] != 0.0f || m[10] != 0.0f || m[11] != 0.0f || m[12] != 0.0f || m[13] != 0.0f) extras |= 1; }
    } else if (p0.flags & GFW_FLAG_HAS_IBIS_DATA) {
        extras |= 1;
    }
    // source_rect map constants: u * pw / W  (cpu_undistort.rs:511-514 with frame_size = (width, height))
    // (frame_size: the source frame, turned by input_rotation — cpu_undistort.rs:484-490; fill_common evaluates the same expression for the kernels' uniforms)
    float Wf = (float)p0.width, Hf = (float)p0.height;
    if (p0.input_rotation != 0.0f) {
        if (extras & (8 | 16 | 32)) return false;                       // with the lens-correction blend, margin feather or the Sony mesh: per plane
        GfwCommon rc; fill_common(c, &p0, nullptr, nullptr, 0, rc);
        Wf = rc.frame_w; Hf = rc.frame_h;
        if (!(Wf >= 1.0f) || !(Hf >= 1.0f)) return false;
    }
    if (!map_const_valid(Wf) || !map_const_valid(Hf)) return false;

    // bicubic / Lanczos4 taps of single-channel integer planes are fetched as aligned dwords at 32-bit offsets from the plane base (taps_inside): the base itself
    // must be dword aligned (every allocator's is; a caller's odd sub-buffer goes the per-plane way)
    auto src_off = [&](int i) { return (int64_t)params[i].source_rect[1] * params[i].stride + (int64_t)params[i].source_rect[0] * params[i].bytes_per_pixel; };
    auto dst_off = [&](int i) { return (int64_t)params[i].output_rect[1] * planes[i].output.stride + (int64_t)params[i].output_rect[0] * params[i].bytes_per_pixel; };
    if (p0.interpolation != 2 && bytes_per_sample != 4)
        for (int i = 0; i < nplanes; ++i) if (((uintptr_t)launches[i].src + (uintptr_t)src_off(i)) & 3u) return false;
    memset(&Y, 0, sizeof(Y));
    for (int i = 0; i < nplanes; ++i) {
        GfwYuvPlane &P = Y.pl[i];
        P.src = launches[i].src + src_off(i); P.dst = launches[i].dst + dst_off(i);            // the rect's first pixel (a buffer without rects: the buffer's)
        P.src_stride = params[i].stride; P.dst_stride = planes[i].output.stride;
        P.w = in_w(i); P.h = in_h(i);
        P.org_x = (float)params[i].source_rect[0]; P.org_y = (float)params[i].source_rect[1];
        P.ox32 = 32 * params[i].source_rect[0]; P.oy32 = 32 * params[i].source_rect[1];
        for (int ch = 0; ch < 4; ++ch) P.bg[ch] = params[i].background[ch] * params[i].max_pixel_value;
        P.limit = params[i].pixel_value_limit;
        P.fix = (params[i].flags & GFW_FLAG_FIX_COLOR_RANGE) ? (params[i].plane_index == 0 ? 1 : 2) : 0;
        {   // (what is left of the declared lengths behind the rebased pointers: audit mode range-checks against them)
            const uint64_t sl = planes[i].input.len > (uint64_t)src_off(i) ? planes[i].input.len - (uint64_t)src_off(i) : 0, dl = planes[i].output.len > (uint64_t)dst_off(i) ? planes[i].output.len - (uint64_t)dst_off(i) : 0;
            P.src_len = (int32_t)(sl < 0x7fffffffull ? sl : 0x7fffffffull);
            P.dst_len = (int32_t)(dl < 0x7fffffffull ? dl : 0x7fffffffull);
        }
    }
    Y.nplanes = nplanes;
    Y.width = p0.width; Y.height = p0.height;
    Y.out_w = p0.output_width; Y.out_h = p0.output_height;
    Y.cw = (p0.output_width + dw - 1) / dw; Y.ch = (p0.output_height + dh - 1) / dh;
    Y.matrix_count = matrix_count;
    Y.hrs = (p0.flags & GFW_FLAG_HORIZONTAL_RS) ? 1 : 0;
    Y.background_mode = p0.background_mode;
    Y.model = c->model;
    Y.extras = extras;
    Y.k_all_zero = (p0.k[0] == 0.0f && p0.k[1] == 0.0f && p0.k[2] == 0.0f && p0.k[3] == 0.0f) ? 1 : 0;
    Y.hstretch = p0.input_horizontal_stretch; Y.vstretch = p0.input_vertical_stretch;
    Y.hstretch_div = hdiv ? 1 : 0; Y.vstretch_div = vdiv ? 1 : 0;
    Y.fill_bg = (p0.flags & GFW_FLAG_FILL_WITH_BACKGROUND) ? 1 : 0;
    Y.fix_range = (p0.flags & GFW_FLAG_FIX_COLOR_RANGE) ? 1 : 0;
    Y.rot_on = p0.input_rotation != 0.0f ? 1 : 0;
    memcpy(Y.f, p0.f, sizeof(Y.f)); memcpy(Y.c, p0.c, sizeof(Y.c)); memcpy(Y.k, p0.k, sizeof(Y.k));
    Y.t2[0] = p0.translation2d[0]; Y.t2[1] = p0.translation2d[1];
    Y.r_limit_sq = p0.r_limit * p0.r_limit;
    Y.map_lx = GfwMapConst{(float)in_w(0), Wf, 1.0f / Wf};
    Y.map_ly = GfwMapConst{(float)in_h(0), Hf, 1.0f / Hf};
    if (nplanes >= 2) {
        Y.map_cx = GfwMapConst{(float)in_w(1), Wf, 1.0f / Wf};
        Y.map_cy = GfwMapConst{(float)in_h(1), Hf, 1.0f / Hf};
    }
    Y.kp = p0;
    Y.grid_limit = c->tune_grid > 0 ? c->tune_grid : c->num_cus * 6;
    Y.ablate = 0;                                                             // (reserved: the timing ablations live in GFW_TESTING builds of the kernel source only, gfw_frame.hip)
    S.taps = p0.interpolation;
    return true;
}
static ClipFlavour flavour_of(const ClipBatch *b);      // (gfw_api_clip.inc)
static int tiles_y_of(const GfwYuvArgs &Y, int rb) { return (Y.ch + 4 * rb - 1) / (4 * rb); }      // rows of tiles: each 4 x rb rows of the chroma height
// `pending`: the frames held for a clip launch on this context, sent first if the first pass's table has to be rebuilt (the error returned is that launch's)
static int build_yuv_args(gfw_ctx *c, const FrameIn &F, const GfwPlane *launches, ClipBatch *pending, GfwYuvArgs &Y, FusedShape &S, bool &served) {
    const float *h_matrices = c->matrices_on_device ? nullptr : F.matrices;
    served = fused_eligible(c, F, launches, h_matrices, Y, S);
    if (!served) return GFW_OK;
    const gfw_kernel_params &p0 = F.params[0];
    bool fast1 = false;
    // (a launch of the moving-lens flavour takes the exact first pass: the certified pass's table, p1_f / p1_c and the envelope are functions of the lens)
    if (!Y.extras && flavour_of(pending) != CLIP_MOVING_LENS && p0.output_width <= 65535 && p0.output_height <= 65535) {               // deferred pixels are parked as (x | y << 16)
        const int rc = p1_setup(c, p0, h_matrices, F.matrix_count, pending, Y, fast1); if (rc != GFW_OK) return rc;
    }
    S.fast1 = fast1 ? 1 : 0;
    Y.tiles_x = (Y.cw + 63) / 64; Y.tiles_y = tiles_y_of(Y, gfw_yuv_rows_per_lane(fast1, Y.audit ? 0 : c->tune_rb));
    return GFW_OK;
}

