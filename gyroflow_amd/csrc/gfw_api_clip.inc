// gfw_api_clip.inc — part of gfw_api.hip (textually included): the frames of one launch of the specialised kernel, where they need a context or the runtime —
// ClipBatch, the checksum table of a launch, the staging of a moving-lens launch, the launch itself, flush / append / end.  How a launch is described and
// assembled, and which frames may share one, is gfw_clip_host.h's.  Nothing here is a translation unit of its own.

// Frames of one clip call (or frames held from per-plane calls) waiting to go out in one launch of the specialised kernel: the argument block they share — that of
// the frame that opened the launch — and what each brings (gfw_clip_host.h).
struct ClipBatch {
    ClipFlavour flavour = CLIP_SHARED;
    GfwYuvArgs Y;
    ClipFrame fr[GFW_CLIP_MAX] = {};
    hipFunction_t fn = nullptr;
    int grid = 0, n = 0;
    int n_call = 0;                              // frames of the clip call being dealt into launches (0: frames held from per-plane calls)
    int limit = GFW_CLIP_MAX;                    // frames this launch takes: clip_launch_limit() of the frame that opened it
    const gfw_buffers *first = nullptr;          // planes of the frame that opened the pending launch (fully validated by run_planes)
    const char *backend = "";
    // CLIP_PER_FRAME: the first-pass table is sized once for the envelope of the call's frames (p1_setup: the largest corner-ray half-extents over their fov and translation2d)
    double env_hx = 0.0, env_hy = 0.0;
    ClipBatch() {}
    // The batch of a clip call (and of the gfw_debug_jit_key_clip_* hooks, which answer what that call would launch)
    ClipBatch(ClipFlavour fl, int n_frames, int nplanes, const gfw_kernel_params *params) : flavour(fl), n_call(n_frames) {
        double hx, hy;
        for (int f = 0; fl == CLIP_PER_FRAME && f < n_frames; ++f) { p1_corner_extent(params[(size_t)f * nplanes], hx, hy); env_hx = fmax(env_hx, hx); env_hy = fmax(env_hy, hy); }
    }
};
static ClipFlavour flavour_of(const ClipBatch *b) { return b ? b->flavour : CLIP_SHARED; }      // (no batch: a frame on its own)
static void clip_envelope(const ClipBatch *b, double &hx, double &hy) { if (flavour_of(b) == CLIP_PER_FRAME) { hx = fmax(hx, b->env_hx); hy = fmax(hy, b->env_hy); } }
// gfw_set_frame_checksums: the word of the next frame submitted on the context (nullptr: off)
// (peek: the ring index advances — sum_commit — only once the frame has been enqueued; a call that fails consumes no slot, so "frame k submitted" keeps meaning what gfwarp.h says)
static unsigned long long *next_sum(gfw_ctx *c) { return (c->sums && c->sum_n) ? c->sums + (c->sum_k % c->sum_n) : nullptr; }
static void sum_commit(gfw_ctx *c, unsigned long long *sum) { if (sum) c->sum_k++; }
// The cap of clip_frames_per_launch: GFW_CLIP_LAUNCH_MB, else 1.1 GB (sixteen 4K 16-bit 4:2:2 frames, four 8K ones)
static size_t clip_launch_bytes() {
    static const size_t v = [] { const char *e = getenv("GFW_CLIP_LAUNCH_MB"); const long mb = e ? atol(e) : 0; return mb > 0 ? (size_t)mb << 20 : (size_t)1100 << 20; }();
    return v;
}
static int clip_launch_limit(const GfwYuvArgs &Y, int nplanes, int n_call) {
    size_t bytes = 0;
    for (int i = 0; i < nplanes && i < 4; ++i) {     // source rows of the plane + destination rows of its OUTPUT (a scaled render's differ: 1080p -> 4K writes four times what it reads)
        const size_t out_rows = (size_t)(i == 0 ? Y.out_h : Y.ch);
        bytes += (size_t)(Y.pl[i].src_stride < 0 ? -Y.pl[i].src_stride : Y.pl[i].src_stride) * (size_t)Y.pl[i].h + (size_t)(Y.pl[i].dst_stride < 0 ? -Y.pl[i].dst_stride : Y.pl[i].dst_stride) * out_rows;
    }
    return clip_frames_per_launch(bytes, clip_launch_bytes(), n_call);
}
// the launch's table of partial sums: one word per frame, workgroup and wave (gfw_frame.hip ck_flush)
static int clip_flush(gfw_ctx *c, ClipBatch *b);
static int ck_table(gfw_ctx *c, int grid, GfwYuvArgs &Y, ClipBatch *pending) {
    const size_t need = (size_t)GFW_CLIP_MAX * (size_t)(grid > 4096 ? grid : 4096) * 4 * sizeof(unsigned long long);      // (2 MB: every grid the launcher picks on 256 CUs)
    if (need > c->d_ck_part.cap && pending && pending->n > 0) { const int frc = clip_flush(c, pending); if (frc != GFW_OK) return frc; }     // (a pending launch names the table that is about to move)
    HIP_TRY(c->d_ck_part.ensure(need), GFW_ERR_HIP);
    Y.ck_part = (unsigned long long *)c->d_ck_part.ptr;
    return GFW_OK;
}
static int ck_finish(gfw_ctx *c, unsigned long long *ck_part, int grid, const ClipFrame *fr, int n) {
    GfwCkSums S; for (int i = 0; i < 16; ++i) S.sum[i] = i < n ? fr[i].sum : nullptr;
    HIP_TRY(gfw_launch_ck_finish(ck_part, grid * 4, n, S, c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
static bool clip_ring_table(gfw_ctx *c, const float *m) {          // a table of gfw_build_matrices' cross-stream ring (ordered by events)
    for (int i = 0; i < gfw_ctx::kBuiltSlots; ++i) if (c->bslots[i].buf.ptr == (const void *)m && c->bslots[i].built.recorded()) return true;
    return false;
}
// diagnosis (GFW_JIT_DEFS=GFW_TIMELINE=1 builds): the per-wave clocks of the 40th launch of a specialised kernel go to $GFW_TIMELINE_FILE (tools/analyze_timeline.py)
static void timeline_dump(gfw_ctx *c, hipFunction_t fn) {
    static const char *tl_file = getenv("GFW_TIMELINE_FILE");
    static int n_launch = 0;
    if (tl_file && ++n_launch == 40) {
        std::vector<unsigned long long> host(8192 * 8);
        (void)hipStreamSynchronize(c->stream);
        if (gfw_jit_read_symbol(fn, "gfw_tl", host.data(), host.size() * 8))
            if (FILE *f = fopen(tl_file, "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
        if (gfw_jit_read_symbol(fn, "gfw_tl_blocks", host.data(), host.size() * 8))       // GFW_TIMELINE = 2 builds: the clocks of the branch-free row's blocks
            if (FILE *f = fopen((std::string(tl_file) + ".blocks").c_str(), "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
    }
}
// The lens slots and the meshes of one moving-lens launch, staged through the context's ring (gfw_hostmem.h) in the layout of clip_lens_layout.  Each launch in
// flight has a slot of the ring to itself — the host waits for a slot's last reader before it refills it —, and the copy is enqueued on the context's stream ahead
// of the launch: a later launch's staging cannot disturb what an earlier, still-running one reads.  The caller records free_again behind the launch.
static int lens_stage(gfw_ctx *c, const ClipFrame *fr, int n, StagedBlock &B) {
    HIP_TRY(c->lens_ring.acquire(GFW_LENS_BLOCK_BYTES, c->stream, &B.slot), GFW_ERR_HIP);
    LensBlockLayout L;
    const int bad = clip_lens_layout(fr, n, B.d(), (GfwLensSlot *)B.h(), L);
    if (bad >= 0) { set_error("frame %d of the launch: mesh of %d values", bad, fr[bad].lens.mesh_len); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
    for (int i = 0; i < L.n_mesh; ++i) memcpy(B.h() + clip_lens_mesh_at(i), fr[L.src[i]].mesh_h, (size_t)fr[L.src[i]].lens.mesh_len * sizeof(float));
    HIP_TRY(B.upload(L.bytes, c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
// One launch of the specialised kernel `fn` of flavour `fl` (the profile bracket is the caller's): the n frames of `fr` under the argument block Y
static int clip_launch(gfw_ctx *c, hipFunction_t fn, int grid, ClipFlavour fl, const GfwYuvArgs &Y, const ClipFrame *fr, int n) {
    StagedBlock B;
    if (fl == CLIP_MOVING_LENS) { const int src = lens_stage(c, fr, n, B); if (src != GFW_OK) return src; }
    GfwClipArgsPL A;
    const size_t bytes = clip_args(A, fl, Y, fr, n, fl == CLIP_MOVING_LENS ? (const GfwLensSlot *)B.d() : nullptr);
    hipError_t e = gfw_jit_launch(fn, &A, bytes, grid, c->stream);
    if (e == hipSuccess && fl == CLIP_MOVING_LENS) e = B.free_again(c->stream);
    int rc = (e == hipSuccess && Y.checksum) ? ck_finish(c, Y.ck_part, grid, fr, n) : GFW_OK;
    if (e != hipSuccess) { set_error("clip launch failed: %s", hipGetErrorString(e)); rc = GFW_ERR_HIP; }
    timeline_dump(c, fn);
    return rc;
}
static int clip_flush(gfw_ctx *c, ClipBatch *b) {
    if (!b || b->n == 0) return GFW_OK;
    prof_begin(c);
    const int rc = clip_launch(c, b->fn, b->grid, b->flavour, b->Y, b->fr, b->n);
    prof_end(c, b->n);
    b->n = 0;
    return rc;
}
// A frame joins the pending launch (opened by run_planes: join_launch): what it brings under the launch's flavour.  A full launch leaves.
static int clip_append(gfw_ctx *c, ClipBatch *b, const ClipFrame &F) {
    sum_commit(c, F.sum);                             // the frame is part of the pending launch from here on
    clip_frame_put(b->fr[b->n++], F, b->flavour);
    c->last_backend = b->backend;
    return b->n >= b->limit ? clip_flush(c, b) : GFW_OK;
}
// The end of a clip call, after a frame's error (`rc`: reported whatever else happens) or after the last frame: what is pending leaves, and GFW_OPT_SYNCHRONOUS
// means what it means for gfw_undistort_frame — a frame that joined a clip launch left run_planes before its own synchronisation point (round-3 advisor finding)
static int clip_end(gfw_ctx *c, ClipBatch *b, int rc) {
    const int frc = clip_flush(c, b);
    const hipError_t e = c->synchronous ? hipStreamSynchronize(c->stream) : hipSuccess;
    if (rc != GFW_OK) return rc;
    if (e != hipSuccess && frc == GFW_OK) { set_error("hipStreamSynchronize failed: %s", hipGetErrorString(e)); return GFW_ERR_HIP; }
    return frc;
}
