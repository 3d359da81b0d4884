// gfw_api_clip.inc — part of gfw_api.hip (textually included): the frames of one launch of the specialised kernel — ClipBatch, what a launch takes, the checksum
// table of a launch, which frames may share one, the launch itself.  Split out of gfw_api.hip in round 6 (the round-5 verdict's hygiene item); nothing here is a
// translation unit of its own.

// Frames of one gfw_undistort_clip call waiting to go out in one launch of the specialised kernel.
static_assert(GFW_CLIP_MAX == GFW_CLIP_FRAMES_MAX, "gfw_frame.h and gfwarp.h disagree on the frames of a clip launch");
struct ClipBatch {
    GfwClipArgs CA;
    hipFunction_t fn = nullptr;
    int grid = 0, n = 0;
    int n_call = 0;                              // frames of the gfw_undistort_clip call being dealt into launches (0: frames held from per-plane calls)
    int limit = GFW_CLIP_MAX;                    // frames this launch takes: clip_launch_limit() of the frame that opened it
    const gfw_buffers *first = nullptr;          // planes of the frame that opened the pending launch (fully validated by run_planes)
    const char *backend = "";
    unsigned long long *sums[GFW_CLIP_MAX] = {};   // gfw_set_frame_checksums: where each frame's checksum goes (the launch's kernel takes it: CA.Y.checksum)
    // gfw_undistort_clip_params: every frame brings its own KernelParams.  Its launches take the per-frame flavour of the specialised kernel (GFW_JIT_PERFRAME),
    // pf[k] is frame k's slot, and the first-pass table is sized once for the envelope of the call's frames (p1_setup: env_hx / env_hy, the largest
    // corner-ray half-extents over the frames' fov and translation2d)
    bool perframe = false;
    GfwFramePer pf[GFW_CLIP_MAX] = {};
    double env_hx = 0.0, env_hy = 0.0;
    // gfw_undistort_clip_lens: every frame brings its own lens and mesh as well.  Its launches take the moving-lens flavour (GFW_JIT_PERFRAME=2), ls[k] is frame k's
    // lens slot and mesh_h[k] its mesh on the host (nullptr: none, or already on the device — a frame launched alone names the context's d_mesh); slots and
    // meshes are staged to the device per launch (lens_stage).  The flavour takes the exact first pass, so there is no envelope.
    bool lens = false;
    GfwLensSlot ls[GFW_CLIP_MAX] = {};
    const float *mesh_h[GFW_CLIP_MAX] = {};
};
static bool clip_lens_flavour(const ClipBatch *b) { return b && b->lens; }
static int clip_flavour(const ClipBatch *b) { return !b ? 0 : b->lens ? 2 : b->perframe ? 1 : 0; }
static void clip_envelope(const ClipBatch *b, double &hx, double &hy) {
    if (b && b->perframe) { hx = fmax(hx, b->env_hx); hy = fmax(hy, b->env_hy); }
}
// The batch of a gfw_undistort_clip_params call (and of gfw_debug_jit_key_clip_params, which answers what that call would launch): the per-frame flavour, and the
// first-pass table's envelope — the call knows every frame's fov and zoom centre, so the table is sized once for all of them (p1_setup)
static void clip_params_batch(ClipBatch &b, int n_frames, int nplanes, const gfw_kernel_params *params) {
    b.n_call = n_frames; b.perframe = true;
    for (int f = 0; f < n_frames; ++f) {
        double hx, hy;
        p1_corner_extent(params[(size_t)f * nplanes], hx, hy);
        b.env_hx = fmax(b.env_hx, hx); b.env_hy = fmax(b.env_hy, hy);
    }
}
// What a launch takes of each frame — its planes' pointers and its matrix table —, from the frame's own argument block
static GfwFrameDyn frame_dyn(const GfwYuvArgs &Y) {
    GfwFrameDyn F;
    for (int i = 0; i < 4; ++i) { F.src[i] = Y.pl[i].src; F.dst[i] = Y.pl[i].dst; }
    F.matrices = Y.matrices;
    return F;
}
// A frame's slot of a per-frame launch: what FrameTransform::at_timestamp and the render loop move from frame to frame (DESIGN.md section 3.2a)
static GfwFramePer frame_slot(const GfwYuvArgs &Y) {
    GfwFramePer F;
    F.t2[0] = Y.t2[0]; F.t2[1] = Y.t2[1];
    F.fov = Y.kp.fov; F.lens_correction_amount = Y.kp.lens_correction_amount;
    F.background_margin = Y.kp.background_margin; F.background_margin_feather = Y.kp.background_margin_feather;
    F.fill_bg = Y.fill_bg; F.pad_ = 0;
    return F;
}
// A frame's lens slot of a moving-lens launch: what get_lens_data_at_timestamp, the refraction keyframe and mesh_correction[frame] move (DESIGN.md section 3.2a).
// `mesh`: as the kernel is to read it — a device address, or nullptr for lens_stage to fill in once the launch's meshes have their place
static GfwLensSlot lens_slot(const GfwYuvArgs &Y, const float *mesh, size_t mesh_len) {
    GfwLensSlot F;
    memcpy(F.f, Y.f, sizeof(F.f)); memcpy(F.c, Y.c, sizeof(F.c)); memcpy(F.k, Y.k, sizeof(F.k));
    F.r_limit_sq = Y.r_limit_sq; F.refraction = Y.kp.light_refraction_coefficient;
    F.mesh = mesh; F.mesh_len = (Y.extras & 32) ? (int32_t)mesh_len : 0; F.pad_ = 0;
    return F;
}
// gfw_set_frame_checksums: the word of the next frame submitted on the context (nullptr: off)
// (peek: the ring index advances — sum_commit — only once the frame has been enqueued; a call that fails consumes no slot, so "frame k submitted" keeps meaning what gfwarp.h says)
static unsigned long long *next_sum(gfw_ctx *c) { return (c->sums && c->sum_n) ? c->sums + (c->sum_k % c->sum_n) : nullptr; }
static void sum_commit(gfw_ctx *c, unsigned long long *sum) { if (sum) c->sum_k++; }
// How many frames one launch of the specialised kernel takes.  The frames of a launch are worked through in order by every XCD with no barrier between them, and the
// bytes they touch are in flight together: 8K frames (265 MB read + written each) measured 184 us per frame in launches of 2, 4 or 8 and 200-202 us in launches of
// 16 (4.2 GB per launch); 4K frames (66 MB) 42.3-43.2 us anywhere from 8 to 16 (profiles/r06_c3_frames_per_launch.txt).  So a launch is capped at
// GFW_CLIP_LAUNCH_BYTES of source + destination (1.1 GB: sixteen 4K 16-bit 4:2:2 frames, four 8K ones; never below 2 frames), and the frames of one
// gfw_undistort_clip call are dealt evenly over the launches that needs (16 frames under a cap of 4: 4 + 4 + 4 + 4, not a runt at the end).
static size_t clip_launch_bytes() {
    static const size_t v = [] { const char *e = getenv("GFW_CLIP_LAUNCH_MB"); const long mb = e ? atol(e) : 0; return mb > 0 ? (size_t)mb << 20 : (size_t)1100 << 20; }();
    return v;
}
static int clip_frames_per_launch(size_t bytes_per_frame, size_t budget, int n_call) {     // (also behind gfw_debug_frames_per_launch: tests/test_abi.py)
    const size_t q = bytes_per_frame ? budget / bytes_per_frame : (size_t)GFW_CLIP_MAX;
    int cap = q < 2 ? 2 : (q > (size_t)GFW_CLIP_MAX ? GFW_CLIP_MAX : (int)q);
    if (n_call > cap) { const int launches = (n_call + cap - 1) / cap; cap = (n_call + launches - 1) / launches; }
    return cap;
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
static int ck_finish(gfw_ctx *c, const GfwClipArgs &CA, int grid, unsigned long long *const *sums) {
    GfwCkSums S;
    for (int i = 0; i < 16; ++i) S.sum[i] = i < CA.n_frames ? sums[i] : nullptr;
    HIP_TRY(gfw_launch_ck_finish(CA.Y.ck_part, grid * 4, CA.n_frames, S, c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
static bool clip_same_shape(const gfw_buffers *a, const gfw_buffers *b, int nplanes) {
    for (int i = 0; i < nplanes; ++i) {
        const gfw_buffer_desc *x[2] = {&a[i].input, &a[i].output}, *y[2] = {&b[i].input, &b[i].output};
        for (int k = 0; k < 2; ++k) {
            if (x[k]->width != y[k]->width || x[k]->height != y[k]->height || x[k]->stride != y[k]->stride || x[k]->kind != y[k]->kind ||
                x[k]->len != y[k]->len || x[k]->has_rect != y[k]->has_rect || x[k]->has_rotation != y[k]->has_rotation ||
                memcmp(x[k]->rect, y[k]->rect, sizeof(x[k]->rect)) || x[k]->rotation != y[k]->rotation || !y[k]->data) return false;
        }
    }
    return true;
}
static bool clip_ring_table(gfw_ctx *c, const float *m) {          // a table of gfw_build_matrices' cross-stream ring (ordered by events)
    for (int i = 0; i < gfw_ctx::kBuiltSlots; ++i) if (c->bslots[i].buf.ptr == (const void *)m && c->bslots[i].built.recorded()) return true;
    return false;
}
// The frames of one launch are in flight together, the calls they stand for are ordered: a frame whose planes overlap a pending frame's
// destination (it would read or overwrite that frame's output) or whose destination overlaps a pending frame's source must go out behind them.
// A launch shares ONE argument block among its frames: everything but the per-frame pointers.  The specialised kernel reads a handful of fields from that
// block at run time — plane-0's KernelParams (fov, lens_correction_amount, the refraction coefficient, background margin / feather, the digital lens's
// parameters) and the host-evaluated uniforms (cos / sin of input_rotation, the rotated frame size) — and the jit key blanks them (they may move from
// frame to frame: dynamic zoom, keyframed lens correction).  Frames that arrive through per-plane calls bring their OWN parameters: a frame may join a pending
// launch only when these blocks are byte-identical to the launch's, else the pending frames go out first (gfw_undistort_clip shares one array by contract).
static bool clip_same_params(const GfwYuvArgs &a, const GfwYuvArgs &b) {
    if (memcmp(&a.kp, &b.kp, sizeof(a.kp)) != 0) return false;
    GfwCommon ca = a.common, cb = b.common;
    ca.matrices = cb.matrices = nullptr;              // the per-frame table: carried by GfwFrameDyn
    if (memcmp(&ca, &cb, sizeof(ca)) != 0) return false;
    for (int i = 0; i < 4; ++i) if (a.pl[i].src_len != b.pl[i].src_len || a.pl[i].dst_len != b.pl[i].dst_len) return false;
    return true;
}
// The same for a launch of the per-frame flavour: the argument blocks must agree once the per-frame fields are blanked — in the manner of jit_for's key.  The feature
// bits those fields select (extras: a lens-correction amount below 1, background mode 3, refraction) stay in the comparison, so a frame whose amount reaches 1.0
// opens a new launch (the flavour's kernel is another).
// `lens`: a launch of the moving-lens flavour — the lens, the refraction coefficient and the mesh are blanked as well; k_all_zero and the feature bits (refraction
// on, a mesh present) stay, so a frame that differs there opens a new launch.
static bool clip_same_params_pf(const GfwYuvArgs &a, const GfwYuvArgs &b, bool lens = false) {
    GfwYuvArgs x = a, y = b;
    for (GfwYuvArgs *v : {&x, &y}) {
        v->t2[0] = v->t2[1] = 0.0f; v->fill_bg = 0;
        v->kp.fov = 0.0f; v->kp.lens_correction_amount = 0.0f; v->kp.background_margin = 0.0f; v->kp.background_margin_feather = 0.0f;
        v->kp.translation2d[0] = v->kp.translation2d[1] = 0.0f; v->kp.flags &= ~GFW_FLAG_FILL_WITH_BACKGROUND;
        if (lens) {
            memset(v->f, 0, sizeof(v->f)); memset(v->c, 0, sizeof(v->c)); memset(v->k, 0, sizeof(v->k)); v->r_limit_sq = 0.0f;
            memset(v->kp.f, 0, sizeof(v->kp.f)); memset(v->kp.c, 0, sizeof(v->kp.c)); memset(v->kp.k, 0, sizeof(v->kp.k)); v->kp.r_limit = 0.0f;
            v->kp.light_refraction_coefficient = 0.0f;
            v->common.mesh = nullptr; v->common.mesh_len = 0;
        }
    }
    return clip_same_params(x, y);
}
static bool clip_overlaps(const ClipBatch *b, const gfw_buffers *planes, int nplanes) {
    auto hit = [](const uint8_t *p, size_t pl, const uint8_t *q, size_t ql) { return p && q && p < q + ql && q < p + pl; };
    for (int k = 0; k < b->n; ++k) {
        const GfwFrameDyn &F = b->CA.fr[k];
        for (int i = 0; i < nplanes; ++i) {
            const uint8_t *ns = (const uint8_t *)planes[i].input.data, *nd = (const uint8_t *)planes[i].output.data;
            const size_t nsl = planes[i].input.len, ndl = planes[i].output.len;
            for (int j = 0; j < nplanes && j < 4; ++j) {
                const size_t sl = b->first[j].input.len, dl = b->first[j].output.len;
                if (hit(nd, ndl, F.dst[j], dl) || hit(nd, ndl, F.src[j], sl) || hit(ns, nsl, F.dst[j], dl)) return true;
            }
        }
    }
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
// The lens slots and the meshes of one moving-lens launch, staged through the context's ring (gfw_hostmem.h): a block of GFW_CLIP_MAX slots followed by the launch's
// meshes, GFW_LENS_MESH_STRIDE floats apart.  Consecutive frames that name the same mesh (pointer and length) share one copy of it.  Each launch in flight has a
// slot of the ring to itself — the host waits for a slot's last reader before it refills it —, and the copy is enqueued on the context's stream ahead of the
// launch: a later launch's staging cannot disturb what an earlier, still-running one reads.  The caller records free_again behind the launch.
static int lens_stage(gfw_ctx *c, int n, const GfwLensSlot *ls, const float *const *mesh_h, StagedBlock &B) {
    HIP_TRY(c->lens_ring.acquire(GFW_LENS_BLOCK_BYTES, c->stream, &B.slot), GFW_ERR_HIP);
    GfwLensSlot *h = (GfwLensSlot *)B.h();
    const size_t mesh_at = GFW_CLIP_MAX * sizeof(GfwLensSlot);
    int n_mesh = 0;
    for (int k = 0; k < n; ++k) {
        h[k] = ls[k];
        if (!mesh_h || !mesh_h[k] || ls[k].mesh_len <= 0) continue;
        if (ls[k].mesh_len > GFW_MESH_MAX) { set_error("frame %d of the launch: mesh of %d values", k, ls[k].mesh_len); return GFW_ERR_BUFFER_SIZE_MISMATCH; }
        const bool shared = k > 0 && mesh_h[k - 1] == mesh_h[k] && ls[k - 1].mesh_len == ls[k].mesh_len;
        if (!shared) { memcpy(B.h() + mesh_at + (size_t)n_mesh * GFW_LENS_MESH_STRIDE * sizeof(float), mesh_h[k], (size_t)ls[k].mesh_len * sizeof(float)); ++n_mesh; }
        h[k].mesh = (const float *)(B.d() + mesh_at + (size_t)(n_mesh - 1) * GFW_LENS_MESH_STRIDE * sizeof(float));
    }
    for (int k = n; k < GFW_CLIP_MAX; ++k) memset(&h[k], 0, sizeof(h[k]));
    HIP_TRY(B.upload(mesh_at + (size_t)n_mesh * GFW_LENS_MESH_STRIDE * sizeof(float), c->stream), GFW_ERR_HIP);
    return GFW_OK;
}
// One launch of the specialised kernel (the profile bracket is the caller's).  `pf`: the frames' slots (per-frame flavour) or nullptr; `sums`: used under CA.Y.checksum;
// `ls` / `mesh_h`: the frames' lens slots and host meshes (moving-lens flavour, with `pf`) or nullptr
static int jit_launch(gfw_ctx *c, hipFunction_t fn, int grid, const GfwClipArgs &CA, const GfwFramePer *pf, unsigned long long *const *sums,
                      const GfwLensSlot *ls = nullptr, const float *const *mesh_h = nullptr) {
    hipError_t e;
    if (pf && ls) {
        StagedBlock B;
        { const int src = lens_stage(c, CA.n_frames, ls, mesh_h, B); if (src != GFW_OK) return src; }
        GfwClipArgsPL PL;
        PL.PF.C = CA; memset(PL.PF.fr_pf, 0, sizeof(PL.PF.fr_pf)); memcpy(PL.PF.fr_pf, pf, (size_t)CA.n_frames * sizeof(GfwFramePer));
        PL.lens = (const GfwLensSlot *)B.d();
        e = gfw_jit_launch_pl(fn, PL, grid, c->stream);
        if (e == hipSuccess) e = B.free_again(c->stream);
    } else if (pf) {
        GfwClipArgsPF PF;
        PF.C = CA; memset(PF.fr_pf, 0, sizeof(PF.fr_pf)); memcpy(PF.fr_pf, pf, (size_t)CA.n_frames * sizeof(GfwFramePer));
        e = gfw_jit_launch_pf(fn, PF, grid, c->stream);
    } else e = gfw_jit_launch(fn, CA, grid, c->stream);
    int rc = (e == hipSuccess && CA.Y.checksum) ? ck_finish(c, CA, grid, sums) : GFW_OK;
    if (e != hipSuccess) { set_error("clip launch failed: %s", hipGetErrorString(e)); rc = GFW_ERR_HIP; }
    timeline_dump(c, fn);
    return rc;
}
static int clip_flush(gfw_ctx *c, ClipBatch *b) {
    if (!b || b->n == 0) return GFW_OK;
    b->CA.n_frames = b->n; b->CA.pad_ = 0;
    prof_begin(c);
    const int rc = jit_launch(c, b->fn, b->grid, b->CA, b->perframe ? b->pf : nullptr, b->sums, b->lens ? b->ls : nullptr, b->mesh_h);
    prof_end(c, b->n);
    b->n = 0;
    return rc;
}
// A frame joins the pending launch (opened by run_planes: join_launch): its pointers, its slot in the per-frame flavour, its checksum word.  A full launch leaves.
static int clip_append(gfw_ctx *c, ClipBatch *b, const GfwFrameDyn &D, const GfwFramePer *slot, unsigned long long *sum, const GfwLensSlot *lens = nullptr, const float *mesh_h = nullptr) {
    b->sums[b->n] = sum;
    sum_commit(c, sum);                               // the frame is part of the pending launch from here on
    if (slot) b->pf[b->n] = *slot;
    if (lens) { b->ls[b->n] = *lens; b->mesh_h[b->n] = mesh_h; }
    b->CA.fr[b->n++] = D;
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
