// emu_perlens_driver.inc — TEST INFRASTRUCTURE: one launch of the moving-lens flavour of gfw_jit_kernel (GFW_JIT_PERFRAME=2: gfw_undistort_clip_lens) on the
// fibers — emu_perframe_driver.inc's launch, with the launch's lens slots (GfwClipArgsPL.lens: on the device an array in device memory, here the caller's) as an
// argument
#include "emu_fibers.inc"
#include <vector>

static GfwClipArgsPL emu_clip_args_pl;
static GfwLensSlot emu_lens_slots[GFW_CLIP_MAX];
static void emu_jit_body() { gfw_jit_kernel(emu_clip_args_pl); }

// As gfw_emu_launch_pf (emu_perframe_driver.inc; the flavour has no certified first pass, so no table), plus `lens_slots`: n_frames GfwLensSlot records — frame
// f's f, c, k[12], r_limit_sq, refraction coefficient, mesh pointer and length.  `kp` is the launch's first frame's KernelParams: the clip-constant fields.
extern "C" int gfw_emu_launch_pl(int n_frames, const uint8_t *const *src, uint8_t *const *dst, const float *const *matrices, const void *kp, const void *common, int grid,
                                 const int32_t *plane_ints, const float *plane_floats, const void *slots, const void *lens_slots) {
    if (n_frames < 1 || n_frames > GFW_CLIP_MAX || grid < 8 || (grid & 7) || !slots || !lens_slots) return -1;
    GfwClipArgsPL &PL = emu_clip_args_pl;
    memset(&PL, 0, sizeof(PL));
    GfwClipArgs &C = PL.PF.C;
    C.n_frames = n_frames;
    for (int f = 0; f < n_frames; ++f) {
        for (int p = 0; p < 4; ++p) { C.fr[f].src[p] = src[f * 4 + p]; C.fr[f].dst[p] = dst[f * 4 + p]; }
        C.fr[f].matrices = matrices[f];
    }
    memcpy(PL.PF.fr_pf, slots, (size_t)n_frames * sizeof(GfwFramePer));
    memset(emu_lens_slots, 0, sizeof(emu_lens_slots));
    memcpy(emu_lens_slots, lens_slots, (size_t)n_frames * sizeof(GfwLensSlot));
    PL.lens = emu_lens_slots;
    for (int p = 0; p < 4; ++p) {
        GfwYuvPlane &P = C.Y.pl[p];
        P.src = src[p]; P.dst = dst[p]; P.src_len = 0x7fffffff; P.dst_len = 0x7fffffff;
        if (plane_ints) { P.src_stride = plane_ints[4 * p]; P.dst_stride = plane_ints[4 * p + 1]; P.w = plane_ints[4 * p + 2]; P.h = plane_ints[4 * p + 3]; }
        if (plane_floats) { for (int c = 0; c < 4; ++c) P.bg[c] = plane_floats[5 * p + c]; P.limit = plane_floats[5 * p + 4]; }
    }
    C.Y.matrices = matrices[0];
    if (kp) memcpy(&C.Y.kp, kp, sizeof(C.Y.kp));
    if (common) memcpy(&C.Y.common, common, sizeof(C.Y.common));
    C.Y.common.matrices = matrices[0];
    return emu::run_grid(grid, emu_jit_body);
}
