// test_clip_host.cpp — TEST INFRASTRUCTURE: the host code that describes and assembles a clip launch (gyroflow_amd/csrc/gfw_clip_host.h: the flavours, a frame's
// record, the argument block, which frames may share a launch, the staged block of a moving-lens launch) in a program of its own, built with AddressSanitizer and
// UBSan (tests/test_cpp_clip_host.py; host pass only, no device, no library).  Device addresses are fakes that are never dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/gfwarp.h"
#include "../../gyroflow_amd/csrc/gfw_clip_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
static const char *const D = (const char *)(uintptr_t)0x500000000000ull;     // a "device" address: never dereferenced
static const ClipFlavour FLAVOURS[3] = {CLIP_SHARED, CLIP_PER_FRAME, CLIP_MOVING_LENS};

// An argument block as build_yuv_args would leave it, every field the comparisons look at non-zero
static GfwYuvArgs base_args() {
    GfwYuvArgs Y;
    memset(&Y, 0, sizeof(Y));
    Y.nplanes = 2; Y.extras = 4 | 8 | 32; Y.k_all_zero = 0; Y.model = 1; Y.matrix_count = 7;
    for (int i = 0; i < 4; ++i) { Y.pl[i].src = (const uint8_t *)D + 0x1000 * i; Y.pl[i].dst = (uint8_t *)D + 0x100000 + 0x1000 * i; Y.pl[i].src_len = 4000 + i; Y.pl[i].dst_len = 5000 + i; }
    Y.matrices = (const float *)(D + 0x200000);
    Y.kp.fov = 1.25f; Y.kp.lens_correction_amount = 0.5f; Y.kp.background_margin = 0.1f; Y.kp.background_margin_feather = 0.05f;
    Y.kp.translation2d[0] = 3.0f; Y.kp.translation2d[1] = -2.0f; Y.kp.flags = 16;
    Y.kp.f[0] = 1000.0f; Y.kp.f[1] = 1001.0f; Y.kp.c[0] = 960.0f; Y.kp.c[1] = 540.0f;
    for (int i = 0; i < 12; ++i) Y.kp.k[i] = 0.01f * (float)(i + 1);
    Y.kp.r_limit = 2.5f; Y.kp.light_refraction_coefficient = 1.33f; Y.kp.width = 1920; Y.kp.height = 1080;
    memcpy(Y.f, Y.kp.f, sizeof(Y.f)); memcpy(Y.c, Y.kp.c, sizeof(Y.c)); memcpy(Y.k, Y.kp.k, sizeof(Y.k));
    Y.t2[0] = Y.kp.translation2d[0]; Y.t2[1] = Y.kp.translation2d[1]; Y.r_limit_sq = Y.kp.r_limit * Y.kp.r_limit; Y.fill_bg = 0;
    Y.common.matrices = Y.matrices; Y.common.mesh = (const float *)(D + 0x300000); Y.common.mesh_len = 40; Y.common.digital = 3;
    Y.common.frame_w = 1920.0f; Y.common.frame_h = 1080.0f; Y.common.rot_cos = 1.0f;
    return Y;
}

// ---- the argument block -----------------------------------------------------------------------------------------------------------------------------------------------
static void fill_frames(ClipFrame *fr, int n, unsigned long long *sums) {
    memset(fr, 0, (size_t)n * sizeof(ClipFrame));
    for (int k = 0; k < n; ++k) {
        for (int i = 0; i < 4; ++i) { fr[k].dyn.src[i] = (const uint8_t *)D + 0x10000 * (k + 1) + 0x100 * i; fr[k].dyn.dst[i] = (uint8_t *)D + 0x4000000 + 0x10000 * (k + 1) + 0x100 * i; }
        fr[k].dyn.matrices = (const float *)(D + 0x8000000) + 64 * k;
        fr[k].per.t2[0] = 1.0f + (float)k; fr[k].per.t2[1] = -1.0f - (float)k; fr[k].per.fov = 1.0f + 0.125f * (float)k; fr[k].per.lens_correction_amount = 0.25f * (float)(k % 4);
        fr[k].per.background_margin = 0.5f + (float)k; fr[k].per.background_margin_feather = 0.75f + (float)k; fr[k].per.fill_bg = k & 1;
        fr[k].lens.f[0] = 900.0f + (float)k;
        fr[k].sum = sums + k;
    }
}
static void test_argument_block() {
    const GfwYuvArgs Y = base_args();
    unsigned long long sums[GFW_CLIP_MAX];
    ClipFrame fr[GFW_CLIP_MAX];
    const GfwLensSlot *d_lens = (const GfwLensSlot *)(D + 0x9000000);
    const size_t sizes[3] = {sizeof(GfwClipArgs), sizeof(GfwClipArgsPF), sizeof(GfwClipArgsPL)};
    const GfwFramePer zero_slot = {};
    for (int n : {3, 1, GFW_CLIP_MAX}) {
        fill_frames(fr, n, sums);
        for (int fi = 0; fi < 3; ++fi) {
            const ClipFlavour fl = FLAVOURS[fi];
            GfwClipArgsPL A;
            memset(&A, 0xA5, sizeof(A));
            const size_t bytes = clip_args(A, fl, Y, fr, n, d_lens);
            CHECK(bytes == sizes[fi]);
            const unsigned char *raw = (const unsigned char *)&A;
            for (size_t i = bytes; i < sizeof(A); ++i) if (raw[i] != 0xA5) { CHECK(!"a byte beyond the flavour's block was written"); break; }
            CHECK(memcmp(&A.PF.C.Y, &Y, sizeof(Y)) == 0);
            CHECK(A.PF.C.n_frames == n && A.PF.C.pad_ == 0);
            for (int k = 0; k < n; ++k) CHECK(memcmp(&A.PF.C.fr[k], &fr[k].dyn, sizeof(GfwFrameDyn)) == 0);
            if (fl == CLIP_SHARED) continue;
            for (int k = 0; k < n; ++k) CHECK(memcmp(&A.PF.fr_pf[k], &fr[k].per, sizeof(GfwFramePer)) == 0);
            for (int k = n; k < GFW_CLIP_MAX; ++k) CHECK(memcmp(&A.PF.fr_pf[k], &zero_slot, sizeof(GfwFramePer)) == 0);
            if (fl == CLIP_MOVING_LENS) CHECK(A.lens == d_lens);
        }
    }
    CHECK(sizeof(GfwClipArgs) < sizeof(GfwClipArgsPF) && sizeof(GfwClipArgsPF) < sizeof(GfwClipArgsPL) && sizeof(GfwClipArgsPL) <= 4096);
}

// ---- a frame's record ---------------------------------------------------------------------------------------------------------------------------------------------------
static void test_clip_frame() {
    const GfwYuvArgs Y = base_args();
    static const float mesh[40] = {};
    unsigned long long sum = 0;
    FrameIn In{2, nullptr, nullptr, nullptr, nullptr, 7, mesh, 40};
    const GfwFrameDyn dyn = frame_dyn(Y);
    const GfwFramePer per = frame_slot(Y);
    for (int k = 0; k < 4; ++k) CHECK(dyn.src[k] == Y.pl[k].src && dyn.dst[k] == Y.pl[k].dst);
    CHECK(dyn.matrices == Y.matrices);
    CHECK(per.t2[0] == Y.t2[0] && per.t2[1] == Y.t2[1] && per.fov == Y.kp.fov && per.lens_correction_amount == Y.kp.lens_correction_amount &&
          per.background_margin == Y.kp.background_margin && per.background_margin_feather == Y.kp.background_margin_feather && per.fill_bg == Y.fill_bg && per.pad_ == 0);
    for (ClipFlavour fl : FLAVOURS) for (bool joins : {true, false}) {
        const ClipFrame F = clip_frame(Y, In, fl, joins, &sum);
        CHECK(memcmp(&F.dyn, &dyn, sizeof(dyn)) == 0 && F.sum == &sum);
        if (fl >= CLIP_PER_FRAME) CHECK(memcmp(&F.per, &per, sizeof(per)) == 0);
        if (fl >= CLIP_MOVING_LENS) {
            CHECK(memcmp(F.lens.f, Y.f, sizeof(Y.f)) == 0 && memcmp(F.lens.c, Y.c, sizeof(Y.c)) == 0 && memcmp(F.lens.k, Y.k, sizeof(Y.k)) == 0);
            CHECK(F.lens.r_limit_sq == Y.r_limit_sq && F.lens.refraction == Y.kp.light_refraction_coefficient && F.lens.mesh_len == 40 && F.lens.pad_ == 0);
            // both faces of the mesh: from the host with the launch it joins, or the one already on the device when it leaves alone
            if (joins) CHECK(F.lens.mesh == nullptr && F.mesh_h == mesh);
            else CHECK(F.lens.mesh == Y.common.mesh && F.mesh_h == nullptr);
        }
    }
    GfwYuvArgs N = Y;                                   // no mesh feature: no mesh in the slot, whatever the call brought
    N.extras &= ~32;
    const ClipFrame F = clip_frame(N, In, CLIP_MOVING_LENS, true, nullptr);
    CHECK(F.lens.mesh_len == 0 && F.mesh_h == nullptr && F.lens.mesh == nullptr && F.sum == nullptr);
    // clip_frame_put keeps what the flavour takes
    ClipFrame all = clip_frame(Y, In, CLIP_MOVING_LENS, true, &sum), to;
    for (ClipFlavour fl : FLAVOURS) {
        memset(&to, 0x5A, sizeof(to));
        ClipFrame untouched = to;
        clip_frame_put(to, all, fl);
        CHECK(memcmp(&to.dyn, &all.dyn, sizeof(all.dyn)) == 0 && to.sum == all.sum);
        CHECK(memcmp(&to.per, fl >= CLIP_PER_FRAME ? &all.per : &untouched.per, sizeof(all.per)) == 0);
        CHECK(memcmp(&to.lens, fl >= CLIP_MOVING_LENS ? &all.lens : &untouched.lens, sizeof(all.lens)) == 0);
        CHECK(to.mesh_h == (fl >= CLIP_MOVING_LENS ? all.mesh_h : untouched.mesh_h));
    }
}

// ---- clip_same_params, clip_blank_slots -----------------------------------------------------------------------------------------------------------------------------------
// One difference between two frames' blocks, and the first flavour whose slots carry it (CLIP_SHARED + 3: none does)
struct Diff { const char *name; int carrier; bool in_y; void (*apply)(GfwYuvArgs &); };      // in_y: it touches the block outside kp / common
static const int NO_SLOT = 3;
static const Diff DIFFS[] = {
    {"t2", CLIP_PER_FRAME, true, [](GfwYuvArgs &v) { v.t2[1] += 1.0f; }},
    {"kp.translation2d", CLIP_PER_FRAME, false, [](GfwYuvArgs &v) { v.kp.translation2d[0] += 1.0f; }},
    {"t2 with kp.translation2d", CLIP_PER_FRAME, true, [](GfwYuvArgs &v) { v.t2[0] += 2.0f; v.kp.translation2d[0] += 2.0f; }},
    {"fov", CLIP_PER_FRAME, false, [](GfwYuvArgs &v) { v.kp.fov *= 1.5f; }},
    {"lens_correction_amount", CLIP_PER_FRAME, false, [](GfwYuvArgs &v) { v.kp.lens_correction_amount = 0.75f; }},
    {"background_margin", CLIP_PER_FRAME, false, [](GfwYuvArgs &v) { v.kp.background_margin = 0.2f; }},
    {"background_margin_feather", CLIP_PER_FRAME, false, [](GfwYuvArgs &v) { v.kp.background_margin_feather = 0.3f; }},
    {"fill flag with fill_bg", CLIP_PER_FRAME, true, [](GfwYuvArgs &v) { v.kp.flags |= GFW_FLAG_FILL_WITH_BACKGROUND; v.fill_bg = 1; }},
    {"fill flag", CLIP_PER_FRAME, false, [](GfwYuvArgs &v) { v.kp.flags |= GFW_FLAG_FILL_WITH_BACKGROUND; }},
    {"fill_bg", CLIP_PER_FRAME, true, [](GfwYuvArgs &v) { v.fill_bg = 1; }},
    {"f", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.f[0] += 1.0f; v.kp.f[0] += 1.0f; }},
    {"f alone", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.f[1] += 1.0f; }},
    {"kp.f", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.kp.f[1] += 1.0f; }},
    {"c", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.c[1] += 1.0f; v.kp.c[1] += 1.0f; }},
    {"c alone", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.c[0] += 1.0f; }},
    {"kp.c", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.kp.c[0] += 1.0f; }},
    {"k", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.k[3] += 0.5f; v.kp.k[3] += 0.5f; }},
    {"k alone", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.k[11] += 0.5f; }},
    {"kp.k", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.kp.k[0] += 0.5f; }},
    {"r_limit_sq with kp.r_limit", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.kp.r_limit = 3.0f; v.r_limit_sq = 9.0f; }},
    {"r_limit_sq", CLIP_MOVING_LENS, true, [](GfwYuvArgs &v) { v.r_limit_sq = 9.0f; }},
    {"kp.r_limit", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.kp.r_limit = 3.0f; }},
    {"light_refraction_coefficient", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.kp.light_refraction_coefficient = 1.5f; }},
    {"common.mesh with mesh_len", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.common.mesh += 1024; v.common.mesh_len = 3; }},
    {"common.mesh", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.common.mesh += 1024; }},
    {"common.mesh_len", CLIP_MOVING_LENS, false, [](GfwYuvArgs &v) { v.common.mesh_len = 3; }},
    // no slot's: another launch under every flavour
    {"extras", NO_SLOT, true, [](GfwYuvArgs &v) { v.extras ^= 8; }},
    {"extras (mesh bit)", NO_SLOT, true, [](GfwYuvArgs &v) { v.extras ^= 32; }},
    {"k_all_zero", NO_SLOT, true, [](GfwYuvArgs &v) { v.k_all_zero = 1; }},
    {"src_len", NO_SLOT, true, [](GfwYuvArgs &v) { v.pl[1].src_len += 1; }},
    {"dst_len", NO_SLOT, true, [](GfwYuvArgs &v) { v.pl[0].dst_len += 1; }},
    {"common.digital", NO_SLOT, false, [](GfwYuvArgs &v) { v.common.digital = 4; }},
    {"common.rot_cos", NO_SLOT, false, [](GfwYuvArgs &v) { v.common.rot_cos = 0.5f; }},
    {"kp.input_rotation", NO_SLOT, false, [](GfwYuvArgs &v) { v.kp.input_rotation = 90.0f; }},
};
static void test_same_params() {
    const GfwYuvArgs a = base_args();
    for (ClipFlavour fl : FLAVOURS) CHECK(clip_same_params(a, a, fl));
    for (const Diff &d : DIFFS) {
        GfwYuvArgs b = a;
        d.apply(b);
        CHECK(memcmp(&a, &b, sizeof(a)) != 0);
        for (ClipFlavour fl : FLAVOURS) {
            const bool want = (int)fl >= d.carrier;
            if (clip_same_params(a, b, fl) != want || clip_same_params(b, a, fl) != want) { fprintf(stderr, "clip_same_params: '%s' under flavour %d: expected %s\n", d.name, (int)fl, want ? "equal" : "unequal"); ++failures; }
        }
    }
    {   // the per-frame table is every frame's own
        GfwYuvArgs b = a;
        b.matrices += 256; b.common.matrices += 256;
        for (ClipFlavour fl : FLAVOURS) CHECK(clip_same_params(a, b, fl));
        // ... and so are the planes' pointers
        for (int i = 0; i < 4; ++i) { b.pl[i].src += 64; b.pl[i].dst += 64; }
        for (ClipFlavour fl : FLAVOURS) CHECK(clip_same_params(a, b, fl));
    }
    CHECK(memcmp(&a, &a, sizeof(a)) == 0);
}
// The kernel's key (jit_for): blanked for the flavour, kp and common zeroed but for the digital lens
static void key_of(GfwYuvArgs &K, ClipFlavour fl) {
    clip_blank_slots(K, fl);
    memset(&K.kp, 0, sizeof(K.kp));
    { const int dig = K.common.digital; memset(&K.common, 0, sizeof(K.common)); K.common.digital = dig; }
}
static void test_blanking_for_the_key() {
    const GfwYuvArgs a = base_args();
    for (ClipFlavour fl : FLAVOURS) {
        GfwYuvArgs ka = a, b = a;
        for (const Diff &d : DIFFS) if (d.carrier <= (int)fl) d.apply(b);      // every field the flavour's slots carry differs
        CHECK(fl == CLIP_SHARED || memcmp(&a, &b, sizeof(a)) != 0);
        GfwYuvArgs kb = b;
        key_of(ka, fl); key_of(kb, fl);
        CHECK(memcmp(&ka, &kb, sizeof(ka)) == 0);
        // what stays in the key: everything the kernel is compiled for
        CHECK(ka.extras == a.extras && ka.k_all_zero == a.k_all_zero && ka.common.digital == a.common.digital && ka.nplanes == a.nplanes && ka.pl[2].src_len == a.pl[2].src_len);
        if (fl < CLIP_PER_FRAME) CHECK(memcmp(ka.t2, a.t2, sizeof(a.t2)) == 0);
        if (fl < CLIP_MOVING_LENS) CHECK(memcmp(ka.f, a.f, sizeof(a.f)) == 0 && memcmp(ka.k, a.k, sizeof(a.k)) == 0 && ka.r_limit_sq == a.r_limit_sq);
        // a field no slot of the flavour carries, outside kp / common, is another key
        for (const Diff &d : DIFFS) {
            if (d.carrier <= (int)fl || !d.in_y) continue;
            GfwYuvArgs kc = a;
            d.apply(kc); key_of(kc, fl);
            if (memcmp(&ka, &kc, sizeof(ka)) == 0) { fprintf(stderr, "key: '%s' vanished under flavour %d\n", d.name, (int)fl); ++failures; }
        }
    }
}

// ---- the staged block of a moving-lens launch --------------------------------------------------------------------------------------------------------------------------
static void test_lens_block_layout() {
    std::vector<float> A(GFW_MESH_MAX, 1.0f), B(GFW_MESH_MAX, 2.0f);
    const float *const device_mesh = (const float *)(D + 0x7000000);      // a mesh already on the device: a slot without a host mesh keeps it
    // frame -> (host mesh, length); -1: as the previous copy, >= 0: the index of the copy it opens
    struct Row { const float *mesh; int len; int copy; };
    const Row rows[GFW_CLIP_MAX] = {
        {A.data(), 3, 0}, {A.data(), 3, -1}, {B.data(), 3, 1}, {nullptr, 0, -2}, {B.data(), 3, 2}, {A.data(), 3, 3},
        {A.data(), GFW_MESH_MAX, 4}, {A.data(), GFW_MESH_MAX, -1}, {A.data(), 0, -2}, {A.data(), GFW_MESH_MAX, 5}, {B.data(), GFW_MESH_MAX, 6}, {B.data(), 3, 7},
        {nullptr, 3, -2}, {B.data(), 3, 8}, {B.data(), 3, -1}, {A.data(), 3, 9}};
    ClipFrame fr[GFW_CLIP_MAX];
    memset(fr, 0, sizeof(fr));
    for (int k = 0; k < GFW_CLIP_MAX; ++k) {
        fr[k].lens.f[0] = 100.0f + (float)k; fr[k].lens.mesh_len = rows[k].len; fr[k].mesh_h = rows[k].mesh;
        fr[k].lens.mesh = rows[k].mesh ? nullptr : device_mesh;
    }
    const GfwLensSlot zero_slot = {};
    for (int n : {GFW_CLIP_MAX, 7, 1, 0}) {
        GfwLensSlot slots[GFW_CLIP_MAX];
        memset(slots, 0x5A, sizeof(slots));
        LensBlockLayout L;
        CHECK(clip_lens_layout(fr, n, D, slots, L) == -1);
        int copies = 0, cur = -1;
        for (int k = 0; k < n; ++k) {
            if (rows[k].copy >= 0) { cur = rows[k].copy; CHECK(cur == copies && L.src[cur] == k); ++copies; }
            CHECK(slots[k].f[0] == fr[k].lens.f[0] && slots[k].mesh_len == fr[k].lens.mesh_len);
            if (rows[k].copy == -2) CHECK(slots[k].mesh == fr[k].lens.mesh);      // no mesh from the host: the slot goes through as it came
            else CHECK((const char *)slots[k].mesh == D + GFW_CLIP_MAX * sizeof(GfwLensSlot) + (size_t)cur * GFW_LENS_MESH_STRIDE * 4);
        }
        CHECK(L.n_mesh == copies);
        for (int k = n; k < GFW_CLIP_MAX; ++k) CHECK(memcmp(&slots[k], &zero_slot, sizeof(zero_slot)) == 0);
        CHECK(L.bytes == GFW_CLIP_MAX * sizeof(GfwLensSlot) + (size_t)copies * GFW_LENS_MESH_STRIDE * 4);
        CHECK(L.bytes <= GFW_LENS_BLOCK_BYTES);
        for (int i = 0; i < L.n_mesh; ++i) {      // a copy ends inside its stride, the last one inside the upload
            CHECK(clip_lens_mesh_at(i) + (size_t)fr[L.src[i]].lens.mesh_len * sizeof(float) <= clip_lens_mesh_at(i + 1));
            CHECK(fr[L.src[i]].mesh_h != nullptr);
        }
    }
    CHECK(GFW_MESH_MAX <= GFW_LENS_MESH_STRIDE);
    // sixteen different meshes of the largest size fill the block exactly
    std::vector<std::vector<float>> own(GFW_CLIP_MAX, std::vector<float>(GFW_MESH_MAX, 0.0f));
    for (int k = 0; k < GFW_CLIP_MAX; ++k) { fr[k].mesh_h = own[k].data(); fr[k].lens.mesh_len = GFW_MESH_MAX; fr[k].lens.mesh = nullptr; }
    GfwLensSlot slots[GFW_CLIP_MAX];
    LensBlockLayout L;
    CHECK(clip_lens_layout(fr, GFW_CLIP_MAX, D, slots, L) == -1 && L.n_mesh == GFW_CLIP_MAX && L.bytes == GFW_LENS_BLOCK_BYTES);
    // a mesh longer than a stride holds is refused, with its frame
    fr[5].lens.mesh_len = GFW_MESH_MAX + 1;
    CHECK(clip_lens_layout(fr, GFW_CLIP_MAX, D, slots, L) == 5);
    CHECK(clip_lens_layout(fr, 5, D, slots, L) == -1);
    fr[5].mesh_h = nullptr;                             // (not a host mesh: not this function's to judge)
    CHECK(clip_lens_layout(fr, GFW_CLIP_MAX, D, slots, L) == -1 && L.n_mesh == GFW_CLIP_MAX - 1);
}

// ---- frames in flight together ----------------------------------------------------------------------------------------------------------------------------------------
static void test_overlaps() {
    std::vector<uint8_t> mem(1 << 16);
    uint8_t *m = mem.data();
    const size_t SL = 1000, DL = 2000;
    gfw_buffers first[2];
    memset(first, 0, sizeof(first));
    for (int i = 0; i < 2; ++i) { first[i].input.len = SL; first[i].output.len = DL; }
    // two pending frames of two planes: sources at 0 / 1000 and 2000 / 3000, destinations at 10000 / 12000 and 14000 / 16000
    ClipFrame fr[2];
    memset(fr, 0, sizeof(fr));
    for (int k = 0; k < 2; ++k) for (int i = 0; i < 2; ++i) { fr[k].dyn.src[i] = m + 2000 * k + 1000 * i; fr[k].dyn.dst[i] = m + 10000 + 4000 * k + 2000 * i; }
    auto waits = [&](size_t s0, size_t s1, size_t d0, size_t d1, int n = 2) {
        gfw_buffers p[2] = {first[0], first[1]};
        p[0].input.data = m + s0; p[1].input.data = m + s1; p[0].output.data = m + d0; p[1].output.data = m + d1;
        return clip_overlaps(fr, n, first, p, 2);
    };
    CHECK(!waits(20000, 21000, 30000, 32000));               // apart
    CHECK(!waits(0, 1000, 30000, 32000));                    // source over source: both only read
    CHECK(!waits(2000, 3000, 30000, 32000));
    CHECK(waits(20000, 21000, 30000, 17999));                // destination over a pending destination [16000, 18000) by one byte ...
    CHECK(!waits(20000, 21000, 30000, 18000));               // ... and touching it end to start
    CHECK(waits(20000, 21000, 8001, 32000));                 // [8001, 10001) over the pending destination [10000, 12000) by one byte
    CHECK(!waits(20000, 21000, 8000, 32000));
    CHECK(waits(20000, 21000, 30000, 3999));                 // destination over a pending source [3000, 4000) by one byte
    CHECK(!waits(20000, 21000, 30000, 4000));
    CHECK(waits(9001, 21000, 30000, 32000));                 // source [9001, 10001) over a pending destination by one byte
    CHECK(!waits(9000, 21000, 30000, 32000));
    CHECK(waits(20000, 17999, 30000, 32000));                // ... from behind
    CHECK(!waits(20000, 18000, 30000, 32000));
    CHECK(!waits(20000, 17999, 30000, 32000, 1) && !waits(20000, 21000, 30000, 17999, 1));      // only the pending frames count: the second is not pending here
    CHECK(!waits(20000, 21000, 30000, 17999, 0));
    {   // a plane without a pointer (a launch of fewer than four planes leaves the rest null) hits nothing
        gfw_buffers p[2] = {first[0], first[1]};
        CHECK(!clip_overlaps(fr, 2, first, p, 2));
    }
    // same shape: every description field, and a pointer on every plane
    gfw_buffers a[2], b[2];
    memset(a, 0, sizeof(a));
    for (int i = 0; i < 2; ++i) { a[i].input.width = 64; a[i].input.height = 32; a[i].input.stride = 128; a[i].input.len = 4096; a[i].input.data = m; a[i].output = a[i].input; a[i].output.data = m + 8192; }
    memcpy(b, a, sizeof(a));
    b[0].input.data = m + 100; b[1].output.data = m + 200;
    CHECK(clip_same_shape(a, b, 2));
    b[1].output.stride = 256; CHECK(!clip_same_shape(a, b, 2) && clip_same_shape(a, b, 1)); b[1].output.stride = 128;
    b[0].input.len = 4097; CHECK(!clip_same_shape(a, b, 2)); b[0].input.len = 4096;
    b[1].input.rect[2] = 5; CHECK(!clip_same_shape(a, b, 2)); b[1].input.rect[2] = 0;
    b[1].input.data = nullptr; CHECK(!clip_same_shape(a, b, 2));
}

// ---- frames per launch (the cases of tests/test_abi.py::test_frames_per_launch_of_a_clip_call, which asks the library) ------------------------------------------------------
static void test_frames_per_launch() {
    auto f = [](unsigned long long bytes, unsigned long long budget, int n) { return clip_frames_per_launch((size_t)bytes, (size_t)budget, n); };
    const unsigned long long MB = 1ull << 20, budget = 1100ull << 20;
    const unsigned long long c2 = 3840ull * 2160 * 2 * 2 * 2, c3 = 7680ull * 4320 * 2 * 2 * 2, c1 = 1920ull * 1080 * 3;
    CHECK(f(c2, budget, 16) == 16 && f(c2, budget, 10) == 16 && f(c2, budget, 20) == 10);
    CHECK(f(c3, budget, 16) == 4 && f(c3, budget, 10) == 4 && f(c3, budget, 0) == 4);
    CHECK(f(c1, budget, 16) == 16 && f(c1, budget, 40) == 14);
    CHECK(f(4000 * MB, budget, 16) == 2);
    CHECK(f(0, budget, 7) == 16 && f(c2, 600 * MB, 16) == 8 && f(c2, 600 * MB, 10) == 5);
    for (int n = 1; n < 64; ++n) for (unsigned long long bytes : {c1, c2, c3, 300 * MB}) {
        const int k = f(bytes, budget, n), cap = f(bytes, budget, 0);
        CHECK(2 <= k && k <= cap && cap <= 16);
        if (n <= cap) CHECK(k == cap);
        else {
            const int launches = (n + k - 1) / k;
            CHECK(launches == (n + cap - 1) / cap);      // dealing evenly never costs a launch
            CHECK(k * launches - n < launches);          // ... and the last launch is short by less than one frame per launch
        }
    }
}

static void test_lens_moves() {
    std::vector<gfw_kernel_params> p(6);                 // three frames of two planes: plane 0's params count
    memset(p.data(), 0, p.size() * sizeof(gfw_kernel_params));
    auto none = [](int) { return false; };
    CHECK(!lens_moves(3, 2, p.data(), none) && !lens_moves(0, 2, p.data(), none));
    CHECK(lens_moves(3, 2, p.data(), [](int f) { return f == 2; }));
    p[1].f[0] = 1.0f; p[3].fov = 2.0f; CHECK(!lens_moves(3, 2, p.data(), none));      // (a chroma plane's copy; a per-frame field)
    p[4].k[11] = 1.0f; CHECK(lens_moves(3, 2, p.data(), none) && !lens_moves(2, 2, p.data(), none)); p[4].k[11] = 0.0f;
    p[2].f[1] = 1.0f; CHECK(lens_moves(3, 2, p.data(), none)); p[2].f[1] = 0.0f;
    p[2].c[0] = 1.0f; CHECK(lens_moves(3, 2, p.data(), none)); p[2].c[0] = 0.0f;
    p[4].r_limit = 1.0f; CHECK(lens_moves(3, 2, p.data(), none)); p[4].r_limit = 0.0f;
    p[4].light_refraction_coefficient = 1.0f; CHECK(lens_moves(3, 2, p.data(), none)); p[4].light_refraction_coefficient = 0.0f;
    CHECK(!lens_moves(3, 2, p.data(), none));
}

int main() {
    test_argument_block();
    test_clip_frame();
    test_same_params();
    test_blanking_for_the_key();
    test_lens_block_layout();
    test_overlaps();
    test_frames_per_launch();
    test_lens_moves();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("clip host code ok\n");
    return 0;
}
