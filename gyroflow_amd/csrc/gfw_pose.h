// gfw_pose.h — Almeida pose estimation of a clip's frame pairs on the device (gfw_pose.hip): `PoseAlmeida::estimate_pose`
// (src/core/synchronization/estimate_pose/almeida.rs:23-37) with `solve_ypr_ransac` (:194-238) over `solve_ypr_given` (:124-192), the random draws an input of the call.
#pragma once
#include <hip/hip_runtime.h>
#include "gfw_warp.h"
#include "gfw_pose_math.h"

#define GFW_POSE_LANES 256          // lanes of a workgroup (64 x 4)
#define GFW_POSE_PAIR_MAX 4096      // points of one pair: the best round's inliers are packed as 16-bit indices in 8 KB of LDS
#define GFW_POSE_PAIRS_MAX 65535    // pairs ride on blockIdx.y
#define GFW_POSE_ROUNDS_MAX 1024    // RANSAC rounds of a pair
#define GFW_POSE_STEPS 30           // `(15.0 / ALPHA).ceil()` (:133)

struct GfwPoseArgs {
    const int32_t *pair_first;      // [n_pairs + 1] first point of each pair (device)
    const float *points;            // [2][total][2]: every pair's points of the first frame, then of the second (device)
    const int32_t *triples;         // [n_pairs][num_iters][3] indices into the pair (device)
    const int32_t *sample_first;    // nullptr (every round's list is 0 .. n-1), or [n_pairs + 1] (device)
    const int32_t *samples;         // nullptr, or per pair [num_iters][min(n, num_samples)] (device)
    float4 *pm;                     // [total] (pos.x, pos.y, motion.x, motion.y)            — the prepare stage's, work space
    float4 *rays;                   // [total] (ptx, pty, ok, 0)
    float2 *derivs;                 // [total][3] v1, v2, v3
    float *fits;                    // [n_pairs][num_iters][4] q of every round (w, i, j, k): the caller's round_fits or work space
    int32_t *counts;                // [n_pairs][num_iters] inliers of every round: the caller's round_inliers or work space
    float *quats;                   // [n_pairs][4]
    double *rotations;              // [n_pairs][9]
    int32_t *best;                  // [n_pairs][2] inliers, round
    double K[9];                    // the camera matrix
    float eps_m[27];                // f32(K * E) of the three derivative rotations (roll, pitch, yaw: :69-77), made once by the host
    float vw, vh, fw, fh;           // video size, optical-flow image size as f32
    float cx, cy, fx, fy;           // K cast to f32 (point_angle, :46-57)
    float target;                   // inlier_angle.to_radians()
    int32_t n_pairs, total, num_iters, num_samples;
};

// the prepare stage of `total` points; the fit stage of n_pairs x num_iters lanes; the count stage, a wave per (pair, round); one workgroup per pair.
// Zero-sized launches are skipped.
hipError_t gfw_launch_pose_prepare(const gfw_kernel_params &P, const GfwCommon &C, const GfwPoseArgs &A, hipStream_t s);
hipError_t gfw_launch_pose_fit(const GfwPoseArgs &A, hipStream_t s);
hipError_t gfw_launch_pose_count(const GfwPoseArgs &A, hipStream_t s);
hipError_t gfw_launch_pose_pick(const GfwPoseArgs &A, hipStream_t s);
