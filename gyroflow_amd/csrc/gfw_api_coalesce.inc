// gfw_api_coalesce.inc — plane coalescing: the per-plane calls of a frame held and sent as one fused launch (included by gfw_api.hip: one translation unit)
// ---- plane coalescing (GFW_OPT_COALESCE_PLANES) --------------------------------------------------------------------------------------
// The reference's render loop warps a frame plane by plane: three process_pixels<T> calls (Y, U, V) with the same FrameTransform, each plane through its own
// Stabilization and therefore its own backend object (src/rendering/mod.rs:494-545).  Bound as INTEGRATION.md shows, that is three gfw_undistort_image
// calls on three contexts per frame — which used to mean three launches of the per-plane kernel (373 us per C2 frame) while the fused frame kernel does
// the same work in 46-52.  A PlaneGroup collects those calls: a call that is stream-ordered anyway (asynchronous context, device buffers both sides) is
// validated, copied and held; when the frame's last plane arrives the group goes through run_planes exactly as one gfw_undistort_frame call would —
// on the context that took plane 0 (it owns the clip state: specialised kernel, first-pass table), with every other member's stream ordered behind
// that launch by an event.  Groups are per calling thread; anything else asked of a member context flushes its group first.
struct PendingPlane { gfw_ctx *c; gfw_buffers b; gfw_kernel_params p; int pixel_type; };
struct PlaneGroup {
    std::thread::id thread;
    int n = 0;
    PendingPlane pl[4];
    const float *d_matrices = nullptr;           // device-resident tables (GFW_OPT_MATRICES_ON_DEVICE != 0): the pointer every plane must repeat
    std::vector<float> h_matrices;               // host rows: a copy of plane 0's, which later planes must equal
    int matrix_count = 0, matrices_on_device = 0;
    bool orphan = false;                         // its thread ended in the middle of a frame: deleted by whoever sends the planes on their way
};
static std::mutex g_group_mu;
static std::vector<PlaneGroup *> g_groups;       // at most one per thread that ever coalesced
static std::vector<gfw_ctx *> g_live;            // every context alive (frame_owner links are cleared when their target goes)
// The calling thread's group.  A thread that ends with an empty group takes it along; one that ends in the middle of a frame leaves the planes where the contexts'
// own flushes (gfw_synchronize, gfw_flush, gfw_destroy, the next call) find them.
struct GroupSlot {
    PlaneGroup *g = nullptr;
    ~GroupSlot() {
        if (!g) return;
        std::lock_guard<std::mutex> lk(g_group_mu);
        if (g->n != 0) { g->orphan = true; return; }
        for (size_t i = 0; i < g_groups.size(); ++i) if (g_groups[i] == g) { g_groups[i] = g_groups.back(); g_groups.pop_back(); break; }
        delete g;
    }
};
static thread_local GroupSlot t_slot;
#define t_group (t_slot.g)

// Which contexts are planes of multi-plane frames?  The calling thread's previous gfw_undistort_image call is remembered; a call with the NEXT plane index on
// another context of the same device, lens and matrix count marks both (and through the chain every plane of the frame).  So the first frame of a clip leaves
// plane by plane, and from the second on its calls are held — while a lone Luma / R32f plane (greyscale, a mask, a depth map) is never held waiting for
// siblings that do not exist (round 4 held it until gfw_synchronize: ADVICE r4).
struct LastPlaneCall { gfw_ctx *c = nullptr; int plane_index = -1, matrix_count = 0; bool marked = false; };
static thread_local LastPlaneCall t_last_plane;
static void plane_pattern_note(gfw_ctx *c, const gfw_kernel_params *params, int matrix_count) {
    if (!params) { t_last_plane = LastPlaneCall(); return; }
    LastPlaneCall &L = t_last_plane;
    if (L.c && L.c != c && params->plane_index == L.plane_index + 1 && matrix_count == L.matrix_count && !(c->multi_plane && L.marked)) {    // (nothing to learn once both are marked: no lock)
        std::lock_guard<std::mutex> lk(g_group_mu);
        bool alive = false;
        for (gfw_ctx *m : g_live) alive = alive || m == L.c;
        if (alive && L.c->device == c->device && L.c->model == c->model && L.c->digital == c->digital) { L.c->multi_plane = true; c->multi_plane = true; }
    }
    L.c = c; L.plane_index = params->plane_index; L.matrix_count = matrix_count; L.marked = c->multi_plane;
}
// Orders the streams of the owner's member contexts behind everything enqueued on the owner's stream so far.
static int order_members_behind(gfw_ctx *owner) {
    bool recorded = false;
    for (gfw_ctx *m : g_live) {
        if (m == owner || m->frame_owner != owner || !m->needs_order) continue;
        m->needs_order = false;
        m->last_backend = owner->last_backend;
        if (m->stream == owner->stream) continue;
        if (!recorded) { HIP_TRY(owner->group_done.record(owner->stream), GFW_ERR_HIP); recorded = true; }
        HIP_TRY(owner->group_done.wait_on(m->stream), GFW_ERR_HIP);
    }
    return GFW_OK;
}
// g_group_mu guards the BOOK-KEEPING (the groups, the list of live contexts, the owner links) — not the launches: a frame is detached from its group under the
// lock and sent with the lock released (round 5, ADVICE r4: the lock used to span run_planes, i.e. the first frame's table preparation and, with GFW_OPT_JIT = 2,
// a ~1 s hiprtc build, with every coalescing thread of the process queued behind it).  What runs unlocked touches only the owner context, which the calling
// thread has to itself by the thread-affinity rule of gfwarp.h (the contexts of one frame are one thread's).
typedef std::unique_lock<std::mutex> GroupLock;
struct GroupUnlocked {
    GroupLock &lk;
    explicit GroupUnlocked(GroupLock &l) : lk(l) { lk.unlock(); }
    ~GroupUnlocked() { lk.lock(); }
};
static int clip_flush_on(gfw_ctx *owner) {
    HIP_TRY(select_device(owner->device), GFW_ERR_HIP);
    return clip_flush(owner, owner->held);
}
static int flush_held_frames(gfw_ctx *owner, GroupLock &lk) {
    if (!owner->held || owner->held->n == 0) return GFW_OK;
    int rc;
    { GroupUnlocked u(lk); rc = clip_flush_on(owner); }
    const int orc = order_members_behind(owner);
    return rc != GFW_OK ? rc : orc;
}
// Sends the group through run_planes (as one frame).  g_group_mu is held on entry and on return, released around the launch; `g` may be gone afterwards if it was
// an orphan (the caller's own group never is).
static int group_launch(PlaneGroup *g, GroupLock &lk) {
    if (g->n == 0) return GFW_OK;
    gfw_ctx *owner = g->pl[0].c;
    gfw_buffers local[4]; gfw_kernel_params params[4]; int types[4];
    const int n = g->n;
    gfw_buffers *planes = local;
    // (a synchronous owner — GFW_OPT_FRAME_SYNC — completes its frame before the last plane's call returns; so does a synchronous MEMBER of an asynchronous owner:
    //  its last-plane call synchronises the owner's stream, which must contain the launch by then — ADVICE r5: the frame used to be parked in owner->held)
    bool any_sync = false;
    for (int i = 0; i < g->n; ++i) any_sync = any_sync || g->pl[i].c->synchronous;
    const bool hold_frames = owner->coalesce_frames > 1 && !any_sync;
    if (hold_frames) {
        // the assembled frame may wait for more of its clip — one launch of the specialised kernel for up to coalesce_frames frames, as gfw_undistort_clip
        // issues them; the descriptions a pending launch was validated with must outlive this call
        if (!owner->held) owner->held = new ClipBatch();
        if (owner->held_planes.size() < (size_t)4 * GFW_CLIP_FRAMES_MAX) owner->held_planes.resize((size_t)4 * GFW_CLIP_FRAMES_MAX);
        planes = owner->held_planes.data() + (size_t)4 * (owner->held->n % GFW_CLIP_FRAMES_MAX);
    }
    for (int i = 0; i < n; ++i) { planes[i] = g->pl[i].b; params[i] = g->pl[i].p; types[i] = g->pl[i].pixel_type; }
    // INPUT side of the ordering (round 5): a member context's caller was stream-ordered on THAT context's stream — the upload or decode of its plane, or a
    // consumer still reading its destination, may be in flight there.  The fused launch reads and writes those buffers on the owner's stream: it waits for
    // whatever each member's stream held when the frame was completed (every member's call lies before this point).  Frames held for a clip launch
    // (GFW_OPT_COALESCE_FRAMES) inherit the wait: the launch is enqueued later on the same in-order stream.
    for (int i = 1; i < n; ++i) {
        gfw_ctx *m = g->pl[i].c;
        if (m == owner || m->stream == owner->stream) continue;
        bool seen = false;
        for (int k = 1; k < i; ++k) seen = seen || g->pl[k].c->stream == m->stream;
        if (seen) continue;
        // (the earlier planes' calls have returned GFW_OK: an event that cannot be created, recorded or waited for must not lose their frame — the host waits for
        //  the member's stream instead and the launch goes on; ADVICE r5)
        const bool ordered = m->inputs_ready.record(m->stream) == hipSuccess && m->inputs_ready.wait_on(owner->stream) == hipSuccess;
        if (!ordered) { (void)hipGetLastError(); (void)hipStreamSynchronize(m->stream); }
    }
    for (int i = 1; i < n; ++i) { g->pl[i].c->frame_owner = owner; g->pl[i].c->needs_order = true; }
    for (int i = 0; i < n; ++i) g->pl[i].c->pending_planes.fetch_sub(1, std::memory_order_relaxed);
    // detached: from here on the group is empty (its thread may start the next frame in it, a flush may delete it if orphaned) and the frame is this call's
    const int matrix_count = g->matrix_count;
    std::vector<float> h_matrices;
    const float *mats = g->d_matrices;
    if (!g->matrices_on_device) { h_matrices.swap(g->h_matrices); mats = h_matrices.data(); }
    g->n = 0;
    g = nullptr;
    const FrameIn F = {n, planes, params, types, mats, matrix_count, nullptr, 0};
    int rc;
    {
        GroupUnlocked u(lk);
        if (hold_frames) {
            rc = run_planes(owner, F, owner->held);
            if (rc != GFW_OK || owner->held->n >= owner->coalesce_frames) { const int frc = owner->held->n > 0 ? clip_flush_on(owner) : GFW_OK; if (rc == GFW_OK) rc = frc; }
        } else {
            rc = (owner->held && owner->held->n > 0) ? clip_flush_on(owner) : GFW_OK;      // (frames parked earlier leave first: the calls are ordered)
            if (rc == GFW_OK) rc = run_planes(owner, F);
        }
    }
    if (!(owner->held && owner->held->n > 0)) { const int orc = order_members_behind(owner); if (rc == GFW_OK) rc = orc; }
    return rc;
}
// Everything pending that involves `c`: the frame it is a plane of, the frames it holds as an owner, the frames its owner holds.  g_group_mu held.
static int flush_context_locked(gfw_ctx *c, GroupLock &lk) {
    int rc = GFW_OK;
    for (size_t gi = 0; gi < g_groups.size(); ) {
        PlaneGroup *g = g_groups[gi];
        bool member = false;
        for (int i = 0; i < g->n; ++i) member = member || g->pl[i].c == c;
        if (member) { const int r = group_launch(g, lk); if (rc == GFW_OK) rc = r; gi = 0; continue; }      // (the list may have changed while the lock was released: from the top)
        if (g->orphan && g->n == 0) { g_groups[gi] = g_groups.back(); g_groups.pop_back(); delete g; continue; }      // its thread is gone: nobody else will
        ++gi;
    }
    { const int r = flush_held_frames(c, lk); if (rc == GFW_OK) rc = r; }
    if (c->frame_owner && c->frame_owner != c && c->needs_order) { const int r = flush_held_frames(c->frame_owner, lk); if (rc == GFW_OK) rc = r; }
    return rc;
}
static void gfw_forget_context(gfw_ctx *c) {
    std::lock_guard<std::mutex> lk(g_group_mu);
    if (c->held) { delete c->held; c->held = nullptr; }
    for (size_t i = 0; i < g_live.size(); ++i) if (g_live[i] == c) { g_live[i] = g_live.back(); g_live.pop_back(); break; }
    for (gfw_ctx *m : g_live) if (m->frame_owner == c) { m->frame_owner = nullptr; m->needs_order = false; }
}
static void gfw_register_context(gfw_ctx *c) { std::lock_guard<std::mutex> lk(g_group_mu); g_live.push_back(c); }
