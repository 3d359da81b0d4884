// gfw_clip_host.h — host only: how a clip launch of the specialised kernel is described and assembled — its flavour, what each frame brings to it, the argument
// block, which frames may share a launch, the layout of a moving-lens launch's staged block.  Included behind gfw_frame.h by gfw_api.hip (gfw_api_clip.inc holds
// what needs a context or the runtime); nothing here touches either, and tests/cpp/test_clip_host.cpp holds it in a program of its own.
#pragma once
#include <string.h>
#include <type_traits>
#include "../../include/gfwarp.h"
#include "gfw_frame.h"

#define GFW_MESH_MAX 839   /* MAX_BUFFER_SIZE, gyro_source/splines.rs:88-89 */
static_assert(GFW_CLIP_MAX == GFW_CLIP_FRAMES_MAX, "gfw_frame.h and gfwarp.h disagree on the frames of a clip launch");
// The three argument blocks nest as prefixes of one another: a launch assembles the largest and passes the prefix its flavour's kernel takes (clip_args)
static_assert(offsetof(GfwClipArgsPL, PF) == 0 && offsetof(GfwClipArgsPF, C) == 0, "the clip argument blocks nest as prefixes");
static_assert(std::is_standard_layout<GfwClipArgs>::value && std::is_standard_layout<GfwClipArgsPF>::value && std::is_standard_layout<GfwClipArgsPL>::value, "layout");

// What the frames of a launch bring beside their pointers.  The values are GFW_JIT_PERFRAME's (absent for 0): the kernels' cache names derive from them.
enum ClipFlavour {
    CLIP_SHARED = 0,         // gfw_undistort_clip, frames held from per-plane calls: one argument block for every frame (GfwClipArgs)
    CLIP_PER_FRAME = 1,      // gfw_undistort_clip_params: each frame's KernelParams fields in a GfwFramePer slot (GfwClipArgsPF)
    CLIP_MOVING_LENS = 2,    // gfw_undistort_clip_lens: each frame's lens and mesh in a GfwLensSlot as well, staged to the device per launch (GfwClipArgsPL)
};
// One frame as the entry points take it: gfw_undistort_frame's arguments, a frame of a clip call, the planes a PlaneGroup assembled
struct FrameIn { int nplanes; const gfw_buffers *planes; const gfw_kernel_params *params; const int *pixel_types; const float *matrices; int matrix_count; const float *mesh; size_t mesh_len;
                 bool mesh_checked = false; };      // (gfw_undistort_clip_lens validated the mesh before its first frame)
// What one frame brings to a launch.  Only the parts its launch's flavour takes are filled (clip_frame), kept (clip_frame_put) and sent (clip_args, clip_lens_layout).
struct ClipFrame {
    GfwFrameDyn dyn;                 // its planes' pointers and its matrix table
    GfwFramePer per;                 // CLIP_PER_FRAME and up: its slot
    GfwLensSlot lens;                // CLIP_MOVING_LENS: its lens slot; `mesh` is a device address, or nullptr for clip_lens_layout to fill in once the launch's meshes have their place
    const float *mesh_h;             // ... and its mesh on the host (nullptr: none, or already on the device — a frame launched alone names the context's d_mesh)
    unsigned long long *sum;         // gfw_set_frame_checksums: where its checksum goes (nullptr: off; read under Y.checksum)
};
// What a slot carries is read into it here and blanked, where frames or kernels are compared, by clip_blank_slots.  GfwFrameDyn — the planes' pointers and the matrix table, from the frame's own argument block
inline GfwFrameDyn frame_dyn(const GfwYuvArgs &Y) {
    return GfwFrameDyn{{Y.pl[0].src, Y.pl[1].src, Y.pl[2].src, Y.pl[3].src}, {Y.pl[0].dst, Y.pl[1].dst, Y.pl[2].dst, Y.pl[3].dst}, Y.matrices};
}
// GfwFramePer — what FrameTransform::at_timestamp and the render loop move from frame to frame
inline GfwFramePer frame_slot(const GfwYuvArgs &Y) {
    return GfwFramePer{{Y.t2[0], Y.t2[1]}, Y.kp.fov, Y.kp.lens_correction_amount, Y.kp.background_margin, Y.kp.background_margin_feather, Y.fill_bg, 0};
}
// GfwLensSlot — what get_lens_data_at_timestamp, the refraction keyframe and mesh_correction[frame] move
inline GfwLensSlot lens_slot(const GfwYuvArgs &Y, const float *mesh, size_t mesh_len) {
    GfwLensSlot F;
    memcpy(F.f, Y.f, sizeof(F.f)); memcpy(F.c, Y.c, sizeof(F.c)); memcpy(F.k, Y.k, sizeof(F.k));
    F.r_limit_sq = Y.r_limit_sq; F.refraction = Y.kp.light_refraction_coefficient;
    F.mesh = mesh; F.mesh_len = (Y.extras & 32) ? (int32_t)mesh_len : 0; F.pad_ = 0;
    return F;
}
// The frame of argument block Y, given as In, for a launch of flavour `fl`.  `joins`: it joins a launch being assembled — its mesh comes along from the caller's
// memory and gets its place in the launch's staged block; otherwise it leaves alone and names the mesh on the device that Y does (the context's, uploaded for it).
inline ClipFrame clip_frame(const GfwYuvArgs &Y, const FrameIn &In, ClipFlavour fl, bool joins, unsigned long long *sum) {
    ClipFrame F;
    F.dyn = frame_dyn(Y); F.sum = sum;
    if (fl >= CLIP_PER_FRAME) F.per = frame_slot(Y);
    if (fl >= CLIP_MOVING_LENS) { F.lens = lens_slot(Y, joins ? nullptr : Y.common.mesh, In.mesh_len); F.mesh_h = (joins && (Y.extras & 32)) ? In.mesh : nullptr; }
    return F;
}
inline void clip_frame_put(ClipFrame &to, const ClipFrame &F, ClipFlavour fl) {
    to.dyn = F.dyn; to.sum = F.sum;
    if (fl >= CLIP_PER_FRAME) to.per = F.per;
    if (fl >= CLIP_MOVING_LENS) { to.lens = F.lens; to.mesh_h = F.mesh_h; }
}
// The fields of an argument block that the slots of flavour `fl` carry, blanked: the kernel's copies (Y.*) and the originals they were derived from (Y.kp.*,
// Y.common.*).  The feature bits those fields select (extras: a lens-correction amount below 1, background mode 3, refraction, a mesh present), k_all_zero and
// common.digital are no slot's: a frame that differs there takes another kernel.
inline void clip_blank_slots(GfwYuvArgs &v, ClipFlavour fl) {
    if (fl >= CLIP_PER_FRAME) {
        v.t2[0] = v.t2[1] = 0.0f; v.fill_bg = 0;
        v.kp.fov = 0.0f; v.kp.lens_correction_amount = 0.0f; v.kp.background_margin = 0.0f; v.kp.background_margin_feather = 0.0f;
        v.kp.translation2d[0] = v.kp.translation2d[1] = 0.0f; v.kp.flags &= ~GFW_FLAG_FILL_WITH_BACKGROUND;
    }
    if (fl >= CLIP_MOVING_LENS) {
        memset(v.f, 0, sizeof(v.f)); memset(v.c, 0, sizeof(v.c)); memset(v.k, 0, sizeof(v.k)); v.r_limit_sq = 0.0f;
        memset(v.kp.f, 0, sizeof(v.kp.f)); memset(v.kp.c, 0, sizeof(v.kp.c)); memset(v.kp.k, 0, sizeof(v.kp.k)); v.kp.r_limit = 0.0f;
        v.kp.light_refraction_coefficient = 0.0f; v.common.mesh = nullptr; v.common.mesh_len = 0;
    }
}
// A launch shares ONE argument block among its frames: everything but what the frames bring.  The specialised kernel reads a handful of fields from that block at
// run time — plane-0's KernelParams (fov, lens_correction_amount, the refraction coefficient, background margin / feather, the digital lens's parameters) and the
// host-evaluated uniforms (cos / sin of input_rotation, the rotated frame size) — and the jit key blanks them.  A frame may join a pending launch only when these
// blocks are byte-identical to the launch's once the fields its flavour's slots carry are blanked (CLIP_SHARED: none — gfw_undistort_clip shares one array by
// contract, frames from per-plane calls bring their OWN parameters), else the pending frames go out first.
inline bool clip_same_params(const GfwYuvArgs &a, const GfwYuvArgs &b, ClipFlavour fl) {
    if (fl != CLIP_SHARED) { GfwYuvArgs x = a, y = b; clip_blank_slots(x, fl); clip_blank_slots(y, fl); return clip_same_params(x, y, CLIP_SHARED); }
    if (a.extras != b.extras || a.k_all_zero != b.k_all_zero || memcmp(&a.kp, &b.kp, sizeof(a.kp)) != 0) return false;      // (extras, k_all_zero: what the kernel is compiled for)
    // (the kernel's copies of what the slots carry: functions of `kp` in every block build_yuv_args makes)
    if (memcmp(a.t2, b.t2, sizeof(a.t2)) || a.fill_bg != b.fill_bg || memcmp(a.f, b.f, sizeof(a.f)) || memcmp(a.c, b.c, sizeof(a.c)) || memcmp(a.k, b.k, sizeof(a.k)) ||
        memcmp(&a.r_limit_sq, &b.r_limit_sq, sizeof(float))) return false;
    GfwCommon ca = a.common, cb = b.common;
    ca.matrices = cb.matrices = nullptr;              // the per-frame table: carried by GfwFrameDyn
    if (memcmp(&ca, &cb, sizeof(ca)) != 0) return false;
    for (int i = 0; i < 4; ++i) if (a.pl[i].src_len != b.pl[i].src_len || a.pl[i].dst_len != b.pl[i].dst_len) return false;
    return true;
}
// The planes of `b` are described as those of `a` but for the pointers (gfw_undistort_clip: such a frame needs none of the per-frame validation again)
inline bool clip_same_shape(const gfw_buffers *a, const gfw_buffers *b, int nplanes) {
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
// The frames of one launch are in flight together, the calls they stand for are ordered: a frame whose planes overlap a pending frame's destination (it would
// read or overwrite that frame's output) or whose destination overlaps a pending frame's source must go out behind them.  `first`: the planes of the frame that
// opened the launch, whose lengths are every pending frame's.
inline bool clip_overlaps(const ClipFrame *fr, int n, const gfw_buffers *first, const gfw_buffers *planes, int nplanes) {
    auto hit = [](const uint8_t *p, size_t pl, const uint8_t *q, size_t ql) { return p && q && p < q + ql && q < p + pl; };
    for (int k = 0; k < n; ++k) {
        const GfwFrameDyn &F = fr[k].dyn;
        for (int i = 0; i < nplanes; ++i) {
            const uint8_t *ns = (const uint8_t *)planes[i].input.data, *nd = (const uint8_t *)planes[i].output.data;
            const size_t nsl = planes[i].input.len, ndl = planes[i].output.len;
            for (int j = 0; j < nplanes && j < 4; ++j) {
                const size_t sl = first[j].input.len, dl = first[j].output.len;
                if (hit(nd, ndl, F.dst[j], dl) || hit(nd, ndl, F.src[j], sl) || hit(ns, nsl, F.dst[j], dl)) return true;
            }
        }
    }
    return false;
}
// How many frames one launch of the specialised kernel takes.  The frames of a launch are worked through in order by every XCD with no barrier between them, and the
// bytes they touch are in flight together: 8K frames (265 MB read + written each) measured 184 us per frame in launches of 2, 4 or 8 and 200-202 us in launches of
// 16 (4.2 GB per launch); 4K frames (66 MB) 42.3-43.2 us anywhere from 8 to 16 (profiles/r06_c3_frames_per_launch.txt).  So a launch is capped at `budget` bytes
// of source + destination (never below 2 frames), and the frames of one call are dealt evenly over the launches that needs (16 frames under a cap of 4:
// 4 + 4 + 4 + 4, not a runt at the end).  (Also behind gfw_debug_frames_per_launch: tests/test_abi.py)
inline int clip_frames_per_launch(size_t bytes_per_frame, size_t budget, int n_call) {
    const size_t q = bytes_per_frame ? budget / bytes_per_frame : (size_t)GFW_CLIP_MAX;
    int cap = q < 2 ? 2 : (q > (size_t)GFW_CLIP_MAX ? GFW_CLIP_MAX : (int)q);
    if (n_call > cap) { const int launches = (n_call + cap - 1) / cap; cap = (n_call + launches - 1) / launches; }
    return cap;
}
// Does anything of the lens move over the frames of a call (gfw_undistort_clip_lens; if not, the call is gfw_undistort_clip_params)?  has_mesh(f): frame f has a mesh
template <typename HasMesh>
inline bool lens_moves(int n_frames, int nplanes, const gfw_kernel_params *params, HasMesh has_mesh) {
    for (int f = 0; f < n_frames; ++f) {
        const gfw_kernel_params &p = params[(size_t)f * nplanes], &p0 = params[0];
        if (has_mesh(f) || memcmp(p.f, p0.f, sizeof(p.f)) || memcmp(p.c, p0.c, sizeof(p.c)) || memcmp(p.k, p0.k, sizeof(p.k)) ||
            memcmp(&p.r_limit, &p0.r_limit, sizeof(float)) || memcmp(&p.light_refraction_coefficient, &p0.light_refraction_coefficient, sizeof(float))) return true;
    }
    return false;
}
// The argument block of a launch of `n` frames: assembled in A, of which the kernel of flavour `fl` takes the first bytes — the value returned; nothing behind
// them is written.  `d_lens`: the launch's lens slots on the device (CLIP_MOVING_LENS; not read otherwise).
inline size_t clip_args(GfwClipArgsPL &A, ClipFlavour fl, const GfwYuvArgs &Y, const ClipFrame *fr, int n, const GfwLensSlot *d_lens) {
    GfwClipArgs &C = A.PF.C;
    C.Y = Y; C.n_frames = n; C.pad_ = 0;
    for (int k = 0; k < n; ++k) C.fr[k] = fr[k].dyn;
    if (fl == CLIP_SHARED) return sizeof(GfwClipArgs);
    for (int k = 0; k < GFW_CLIP_MAX; ++k) { if (k < n) A.PF.fr_pf[k] = fr[k].per; else memset(&A.PF.fr_pf[k], 0, sizeof(GfwFramePer)); }
    if (fl == CLIP_PER_FRAME) return sizeof(GfwClipArgsPF);
    A.lens = d_lens; return sizeof(GfwClipArgsPL);
}
// The staged block of a moving-lens launch: GFW_CLIP_MAX lens slots, then n_mesh meshes GFW_LENS_MESH_STRIDE floats apart, mesh i frame src[i]'s; `bytes` to upload
struct LensBlockLayout { int n_mesh, src[GFW_CLIP_MAX]; size_t bytes; };
inline size_t clip_lens_mesh_at(int i) { return GFW_CLIP_MAX * sizeof(GfwLensSlot) + (size_t)i * GFW_LENS_MESH_STRIDE * sizeof(float); }
// Lays the block out for the device address `d_block` and fills its slots on the host, `slots[GFW_CLIP_MAX]`: frame k's, its `mesh` naming the mesh's place in the
// block if it brought one from the host (else kept as it came), zeroes behind the n-th.  Consecutive frames that name the same host mesh (pointer and length)
// share one copy of it.  -> -1, or the first frame whose mesh is longer than GFW_MESH_MAX.
inline int clip_lens_layout(const ClipFrame *fr, int n, const char *d_block, GfwLensSlot *slots, LensBlockLayout &L) {
    L.n_mesh = 0;
    for (int k = 0; k < n; ++k) {
        slots[k] = fr[k].lens;
        if (!fr[k].mesh_h || fr[k].lens.mesh_len <= 0) continue;
        if (fr[k].lens.mesh_len > GFW_MESH_MAX) return k;
        const bool shared = k > 0 && fr[k - 1].mesh_h == fr[k].mesh_h && fr[k - 1].lens.mesh_len == fr[k].lens.mesh_len;
        if (!shared) L.src[L.n_mesh++] = k;
        slots[k].mesh = (const float *)(d_block + clip_lens_mesh_at(L.n_mesh - 1));
    }
    for (int k = n; k < GFW_CLIP_MAX; ++k) memset(&slots[k], 0, sizeof(GfwLensSlot));
    L.bytes = clip_lens_mesh_at(L.n_mesh);
    return -1;
}
