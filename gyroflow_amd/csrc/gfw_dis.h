// gfw_dis.h — DIS dense optical flow of a clip's frame pairs on the device (gfw_dis.hip): the reference's default optical-flow method 2
// (src/core/synchronization/optical_flow/opencv_dis.rs: DISOpticalFlow_PRESET_FAST — patch 8, patch stride 4, 16 descent iterations, finest scale 2, mean-normalised
// patches, spatial propagation), stated in fixed point (tests/_disstmt.py), sampled at the grid points of opencv_dis.rs:62-119 (gfw_flow.hip's grid kernel).
// Variational refinement is NOT part of it: it is gfw_varref.h's, launched behind each level's dense field by gfw_flow_dis_refined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GFW_DIS_PATCH 8             // a patch's side: 64 pixels, a lane each
#define GFW_DIS_STRIDE 4            // between patch origins
#define GFW_DIS_ITERS 16            // proposals of a descent
#define GFW_DIS_LEVELS 9            // levels 0 .. 8: sides <= 8192 give coarsest <= int(log2(8192 / 32) + 0.5) = 8
#define GFW_DIS_SIDE_MAX 8192
#define GFW_DIS_PAIRS_MAX 65535     // pairs ride on blockIdx.y
#define GFW_DIS_FRAMES_MAX 4096     // frames ride on blockIdx.y of the pyramid launches
#define GFW_DIS_NODES_MAX 4096      // grid nodes of a frame (gfw_flow_pyrlk's limit)
#define GFW_DIS_STAGED_MAX ((size_t)1 << 31)       // bytes of one staged block (pairs, host frames)
#define GFW_DIS_WORK_MAX ((size_t)1 << 34)         // bytes of device work space (the pyramids, the dense fields, the patch values)
#define GFW_DIS_DET_MIN 16777216.0f // a patch is descended only above this determinant of its system (times 64^2)
#define GFW_DIS_FAR2 64.0f          // a value further than 8 level pixels from its start value returns to it

struct GfwDisLevel { const uint8_t *base; int64_t frame_bytes; int32_t w, h, stride, pad_; };       // frame f of the level: base + f * frame_bytes
struct GfwDisArgs {
    GfwDisLevel lv[GFW_DIS_LEVELS];    // [0] the caller's frames, [1 .. coarsest] work space (stride = w)
    float *dense[GFW_DIS_LEVELS];       // [finest .. coarsest]: the level's dense field [n_pairs][h_l][w_l][2]
    float *patch[3];                    // the patch values of passes a, b, c of the level in work: [n_pairs][ny nx][2]
    const int32_t *pair_frames;         // [n_pairs][2] (device)
    const float *grid_points;           // [n_frames][grid_nodes][2], the kept nodes of a frame first
    const int32_t *grid_counts;         // [n_frames]
    int32_t *out_pair_first;            // [n_pairs + 1]
    float *points_a, *points_b;         // [sum of the first frames' grid counts][2]
    int32_t coarsest, finest, n_frames, n_pairs, grid_nodes;
};

// Launches of a call, whatever the number of pairs and frames: `coarsest` pyramid levels (all frames each), the grid points (gfw_launch_flow_grid), per level
// coarsest .. finest the three passes and the dense field, then the scan and the node sampling: 3 + coarsest + 4 (coarsest - finest + 1), 24 for 1280 x 720 at the
// reference's finest scale 2.  The per-patch sums of the template are recomputed by each pass's wave (five exact sums of registers it holds anyway) instead of a
// precompute launch and a table; that choice was not measured.  Zero-sized launches are skipped.
hipError_t gfw_launch_dis_pyramid(const GfwDisArgs &A, int level, uint8_t *dst, hipStream_t s);
hipError_t gfw_launch_dis_pass(const GfwDisArgs &A, int level, int pass, hipStream_t s);
hipError_t gfw_launch_dis_dense(const GfwDisArgs &A, int level, hipStream_t s);
hipError_t gfw_launch_dis_scan(const GfwDisArgs &A, hipStream_t s);
hipError_t gfw_launch_dis_nodes(const GfwDisArgs &A, hipStream_t s);
