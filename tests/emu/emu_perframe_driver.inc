// emu_perframe_driver.inc — TEST INFRASTRUCTURE: one launch of the per-frame flavour of gfw_jit_kernel (GFW_JIT_PERFRAME: gfw_undistort_clip_params) on the
// fibers — emu_driver.inc's launch, with the launch's per-frame slots (GfwClipArgsPF.fr_pf) as an argument
#include "emu_fibers.inc"
#include <vector>

static GfwClipArgsPF emu_clip_args_pf;
static void emu_jit_body() { gfw_jit_kernel(emu_clip_args_pf); }
#if defined(EMU_AUDIT) && EMU_AUDIT
// the audit build of the flavour (GFW_JIT_AUDIT=1, bake header GFW_BK_audit (A.audit): what jit_for builds for a per-frame launch under GFW_OPT_KERNEL_VARIANT 3 / 4)
// — every accepted certificate of the first pass re-derived exactly, every tap / store / matrix row / table entry range-checked: counters in emu_audit_words
static unsigned long long emu_audit_words[8];
extern "C" void gfw_emu_audit(unsigned long long *out, int reset) { memcpy(out, emu_audit_words, sizeof(emu_audit_words)); if (reset) memset(emu_audit_words, 0, sizeof(emu_audit_words)); }
#endif

// As gfw_emu_launch (emu_driver.inc), plus `slots`: n_frames GfwFramePer records — frame f's translation2d, fov, lens_correction_amount, background margin and
// feather, fill flag.  `kp` is the launch's first frame's KernelParams (the clip-constant fields; the kernel reads the per-frame ones from the slots).
extern "C" int gfw_emu_launch_pf(int n_frames, const uint8_t *const *src, uint8_t *const *dst, const float *const *matrices, const float *p1_table,
                                 float p1_rho_max, float p1_rho_scale, float p1_eps, float p1_ew, float p1_em, const void *kp, const void *common, int grid,
                                 const int32_t *plane_ints, const float *plane_floats, const float *p1_lat, const void *slots) {
    if (n_frames < 1 || n_frames > GFW_CLIP_MAX || grid < 8 || (grid & 7) || !slots) return -1;
    GfwClipArgsPF &PF = emu_clip_args_pf;
    memset(&PF, 0, sizeof(PF));
    GfwClipArgs &C = PF.C;
    C.n_frames = n_frames;
    for (int f = 0; f < n_frames; ++f) {
        for (int p = 0; p < 4; ++p) { C.fr[f].src[p] = src[f * 4 + p]; C.fr[f].dst[p] = dst[f * 4 + p]; }
        C.fr[f].matrices = matrices[f];
    }
    memcpy(PF.fr_pf, slots, (size_t)n_frames * sizeof(GfwFramePer));
    for (int p = 0; p < 4; ++p) {
        GfwYuvPlane &P = C.Y.pl[p];
        P.src = src[p]; P.dst = dst[p]; P.src_len = 0x7fffffff; P.dst_len = 0x7fffffff;
        if (plane_ints) { P.src_stride = plane_ints[4 * p]; P.dst_stride = plane_ints[4 * p + 1]; P.w = plane_ints[4 * p + 2]; P.h = plane_ints[4 * p + 3]; }
        if (plane_floats) { for (int c = 0; c < 4; ++c) P.bg[c] = plane_floats[5 * p + c]; P.limit = plane_floats[5 * p + 4]; }
    }
    C.Y.matrices = matrices[0];
    C.Y.p1_table = reinterpret_cast<const float2 *>(p1_table);
    C.Y.p1_rho_max = p1_rho_max; C.Y.p1_kmax = GFW_P1_RFORM ? sqrtf(p1_rho_max) : p1_rho_max; C.Y.p1_rform = GFW_P1_RFORM; C.Y.p1_rho_scale = p1_rho_scale; C.Y.p1_eps = p1_eps; C.Y.p1_ew = p1_ew; C.Y.p1_em = p1_em;
    if (p1_lat) for (int i = 0; i < 6; ++i) C.Y.p1_lat[i] = p1_lat[i];
    if (kp) memcpy(&C.Y.kp, kp, sizeof(C.Y.kp));
    if (common) memcpy(&C.Y.common, common, sizeof(C.Y.common));
    C.Y.common.matrices = matrices[0];
#if defined(EMU_AUDIT) && EMU_AUDIT
    C.Y.audit = emu_audit_words;
    for (int p = 0; p < 4; ++p) if (plane_ints) { C.Y.pl[p].src_len = plane_ints[16 + 2 * p]; C.Y.pl[p].dst_len = plane_ints[16 + 2 * p + 1]; }    // (the declared lengths)
#endif
    return emu::run_grid(grid, emu_jit_body);
}
