// gfw_varref.h — the variational refinement of the DIS dense flow's fields on the device (gfw_varref.hip): the Brox-style refinement that the reference's
// DISOpticalFlow_PRESET_FAST (src/core/synchronization/optical_flow/opencv_dis.rs:59) runs on every pyramid level, as Kroeger et al. use it, stated operation by
// operation in tests/_varrefstmt.py.  It is an entry point of its own (gfw_flow_dis_refined) beside gfw_flow_dis, whose interface and rejection of a non-zero
// variational_iters are pinned by its tests and whose kernels' figures are pinned by DESIGN.md 3.2k: the refinement is a translation unit of its own that leaves
// gfw_dis.hip as it is, and this header needs nothing of gfw_dis.h (the host header gfw_varref_host.h makes a level's block from a GfwDisArgs).
//
// The defaults — alpha 20, delta 5, gamma 10, 5 fixed-point and 5 SOR iterations, omega 1.6; zeta 0.1 and eps 0.001 fixed — are the values OpenCV's DIS
// implementation sets TO THE BUILDER'S BEST KNOWLEDGE.  OpenCV's source is not part of the reference tree: nothing in this tree confirms them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GFW_VARREF_ZETA 0.1f            // the data terms' normalisation floor
#define GFW_VARREF_EPS2 0.000001f       // eps^2 under every square root
#define GFW_VARREF_ITERS_MAX 64         // fixed-point and SOR iterations of a level

// The per-pixel planes of the level in work, each f32 [n_pairs][h][w]
enum { GFW_VR_IX, GFW_VR_IY, GFW_VR_IZ, GFW_VR_IXX, GFW_VR_IXY, GFW_VR_IYY, GFW_VR_IXZ, GFW_VR_IYZ,     // prepare: the derivative images
       GFW_VR_DU, GFW_VR_DV,                                                                           // prepare zeroes, the half-sweeps update
       GFW_VR_A11, GFW_VR_A12, GFW_VR_A22, GFW_VR_B1, GFW_VR_B2, GFW_VR_WR, GFW_VR_WD,                  // coeff: the system, the right and down link weights
       GFW_VARREF_PLANES };

// One level of every pair of a call
struct GfwVarrefArgs {
    const uint8_t *base; int64_t frame_bytes;   // the level's images: frame f at base + f * frame_bytes
    int32_t w, h, stride, n_pairs;
    const int32_t *pair_frames;                 // [n_pairs][2] (device)
    float *U;                                   // the level's dense field [n_pairs][h][w][2], refined in place
    float *plane[GFW_VARREF_PLANES];
    float alpha, delta, gamma, omega;
};

// Launches of a level with fixed_point_iters = F > 0 and sor_iters = S, all pairs in each (the pair on blockIdx.y): prepare, F x (coeff, S x (even half-sweep, odd
// half-sweep)), apply — gfw_varref_launches = 2 + F (1 + 2 S), 57 at 5 / 5, on top of the level's four of gfw_dis.h.  1280 x 720 at the finest scale 2 has four
// levels: 24 + 4 x 57 = 252 launches a call.  F = 0: none.  The prepare kernel recomputes the warped image over each pixel's footprint (21 samples) instead of a
// warp launch and a derivative launch over a stored image; apply is a launch of its own (the last half-sweep updates one colour only).  Neither choice was measured.
inline int gfw_varref_launches(int fixed_point_iters, int sor_iters) { return fixed_point_iters > 0 ? 2 + fixed_point_iters * (1 + 2 * sor_iters) : 0; }
hipError_t gfw_launch_varref_prepare(const GfwVarrefArgs &A, hipStream_t s);
hipError_t gfw_launch_varref_coeff(const GfwVarrefArgs &A, hipStream_t s);
hipError_t gfw_launch_varref_sor(const GfwVarrefArgs &A, int colour, hipStream_t s);
hipError_t gfw_launch_varref_apply(const GfwVarrefArgs &A, hipStream_t s);
