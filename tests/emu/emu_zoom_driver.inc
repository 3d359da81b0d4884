// emu_zoom_driver.inc — TEST INFRASTRUCTURE: launches of gfw_zoom_kernel (gfw_zoom.hip, compiled for the host above) on the fibers.  A workgroup of the zoom search has
// GFW_ZOOM_LANES = 64 lanes (one wave); the fibers interpret 256 (64 x 4): the lanes beyond do not exist on the device and leave at once.  The host side is the entry
// points' own (gfw_zoom_host.h): the staged block and FovIterative::new in f32.
#include "emu_fibers.inc"
#include "../../gyroflow_amd/csrc/gfw_zoom_host.h"
[[noreturn]] void emu_unsupported(const char *what) { fprintf(stderr, "emu: %s is not interpreted\n", what); abort(); }

static gfw_kernel_params emu_zP; static GfwCommon emu_zC; static GfwZoomArgs emu_zA;
static std::vector<uint64_t> emu_zblock;
static void emu_zoom_body() {
    if (emu_cur->tid.y >= 1) return;
    if (emu_zC.model == GFW_MODEL_OPENCV_FISHEYE) gfw_zoom_kernel<GFW_MODEL_OPENCV_FISHEYE>(emu_zP, emu_zC, emu_zA);
    else gfw_zoom_kernel<-1>(emu_zP, emu_zC, emu_zA);
}

// The argument block as gfw_zoom_fovs / gfw_zoom_fovs_stab make it: what they stage goes into ONE block of exactly the layout's bytes ("device" = host memory)
static void emu_zoom_stage(const void *kp, const void *common, const GfwTracks &T, const gfw_zoom_search *search, const gfw_zoom_frame *frames, int n_frames,
                           const float *rotations, const gfw_frame_stab *const *stabs, const double *const *meshes, const size_t *mesh_lens,
                           double *fov_minimal, double *debug_points) {
    memcpy(&emu_zP, kp, sizeof(emu_zP)); memcpy(&emu_zC, common, sizeof(emu_zC));
    GfwZoomArgs &A = emu_zA;
    memset(&A, 0, sizeof(A));
    const GfwZoomLayout Z = gfw_zoom_layout(n_frames, rotations != nullptr, stabs != nullptr, stabs ? gfw_stab_points_total(stabs, n_frames) : 0,
                                            meshes != nullptr, meshes ? gfw_zoom_mesh_doubles(meshes, mesh_lens, n_frames) : 0);
    emu_zblock.assign(Z.total / 8, 0);
    char *h = (char *)emu_zblock.data();
    gfw_zoom_fill(Z, frames, n_frames, rotations, stabs, meshes, mesh_lens, h, h, A);
    A.T = T; A.fov_minimal = fov_minimal; A.debug_points = debug_points;
    gfw_zoom_search_args(*search, A);
}

// tracks: 10 pointers / counts as GfwTracks lists them; search, frames: the ABI's
extern "C" int gfw_emu_zoom(const void *kp, const void *common, const int64_t *org_ts, const double *org_q, int org_n, const int64_t *sm_ts, const double *sm_q, int sm_n,
                            const int64_t *off_ts, const double *off_ms, int off_n, double duration_ms, const gfw_zoom_search *search,
                            const gfw_zoom_frame *frames, int n_frames, const float *rotations, double *fov_minimal, double *debug_points) {
    emu_zoom_stage(kp, common, GfwTracks{org_ts, org_q, org_n, sm_ts, sm_q, sm_n, off_ts, off_ms, off_n, duration_ms}, search, frames, n_frames, rotations,
                   nullptr, nullptr, nullptr, fov_minimal, debug_points);
    return emu::run_grid(n_frames, emu_zoom_body);                            // gfw_launch_zoom: one launch, a workgroup per frame
}

// Test-only entry: the fold and the round logic of the kernel source (gfw_zoom_rounds) with the point map replaced by a table — pass 0 answers with outline[i],
// pass k with refined[k - 1][i] — so that constructed polygons drive the loop through each of its exits.
struct EmuZoomTable {
    const float *outline, *refined;
    float2 operator()(int pass, int i, float, float) const {
        const float *p = pass == 0 ? outline + 2 * i : refined + ((size_t)(pass - 1) * GFW_ZOOM_REFINED + i) * 2;
        return float2{p[0], p[1]};
    }
};
static EmuZoomTable emu_zT; static float emu_zw, emu_zh, emu_zmargin, emu_za, emu_zm0;
static float2 emu_zpoly[GFW_ZOOM_RECT]; static int emu_zidx;
static void emu_zoom_table_body() {
    if (emu_cur->tid.y >= 1) return;
    const int t = threadIdx.x;
    const float m0 = gfw_zoom_rounds(emu_zT, t, emu_zw, emu_zh, emu_zmargin, emu_za, emu_zpoly, &emu_zidx, (double *)nullptr);
    if (t == 0) emu_zm0 = m0;
}
extern "C" int gfw_emu_zoom_table(const float *outline, const float *refined, int width, int height, int org_output_width, int org_output_height, float margin, double *fov) {
    emu_zT = EmuZoomTable{outline, refined};
    const gfw_zoom_search search = {width, height, org_output_width, org_output_height, margin, 0};
    GfwZoomArgs A;
    gfw_zoom_search_args(search, A);
    emu_zw = A.w; emu_zh = A.h; emu_zmargin = A.margin; emu_za = A.inv_aspect;
    const int rc = emu::run_grid(1, emu_zoom_table_body);
    if (rc) return rc;
    *fov = (double)(emu_zm0 * 2.0f / A.out_dim0);
    return 0;
}
