// gfw_dis.hip — DIS dense optical flow of a clip's frame pairs (Kroeger et al., "Fast Optical Flow using Dense Inverse Search"), the reference's default optical-flow
// method 2 with the parameters of DISOpticalFlow_PRESET_FAST (src/core/synchronization/optical_flow/opencv_dis.rs:59), sampled at the grid points of :62-119.
// OpenCV's source is not part of the reference tree: the contract is tests/_disstmt.py, the published scheme stated operation by operation.  Variational refinement is
// NOT part of it.  OpenCV's raster-order propagation depends on its thread count and is not reproduced: three synchronous passes, each reading its neighbours from the
// pass before, so no result depends on the order in which workgroups run.
//
// Every sum over a patch's 64 pixels is an INTEGER: gradients are the integer central difference, bilinear samples of the second frame are fixed point (gfw_image.h's
// gfw_image_sample: weights of 14 bits that sum to 16384, 5 fraction bits kept: 0 .. 8160), the difference d against 32 A has |d| <= 8160, a lane's d d <= 2^26
// fits an int32 and a patch's sums fit an int64 with room (64 Sdd <= 2^38); the mean normalisation is formed in integers too (64 Sdd - Sd Sd), and ONE conversion
// to f32 follows.  The order of an exact sum is free, so the wave reduces with 64-bit LDS atomics and the result equals the statement's to the bit.
//
// The inverse search is ONE wave per (patch, pair), a lane per patch pixel: a barrier is a wave barrier.  The template's (A, Ix, Iy) stay in registers over every
// evaluation of the pass; every lane computes the same f32 update from the same sums, so the trip counts are wave-uniform by construction.
//
// NO INDEX OUTSIDE A LEVEL CAN BE FORMED.  A level has sides w, h >= 8 (the host builds no smaller one: min(w, h) >= 8 * 2^coarsest), so nx = (w - 8) / 4 + 1 >= 1 and
// a patch pixel is x = 4 i + (lane & 7) <= 4 (nx - 1) + 7 <= w - 1.  The gradient reads min(x + 1, w - 1) and max(x - 1, 0).  A sample reads columns (gfw_image.h)
// clamp(x + ix, 0, w - 1) and clamp(x + ix + 1, 0, w - 1), ix the integer part of the displacement, itself clamped to +-16384 as a FLOAT before the cast (no cast
// outside the int range is executed; a displacement is finite because det > 2^24 divides finite sums): |x + ix + 1| < 2^15 and the clamp lands in the level.  The dense
// field is read at coordinates clamped to [0, n - 1] before the cast, with the neighbour min(i0 + 1, n - 1).  The pyramid reads 2x + 1 <= 2 (w / 2 - 1) + 1 <= w - 1.
// Rows alike.  Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; control flow around the barriers is workgroup-uniform.
#include <hip/hip_runtime.h>
#include "gfw_dis.h"
#include "gfw_image.h"

// The field U [h][w][2] at (cx, cy), coordinates clamped to the level
__device__ __forceinline__ void gfw_dis_bilinear(const float *U, int w, int h, float cx, float cy, float &vx, float &vy) {
    cx = fminf(fmaxf(cx, 0.0f), (float)(w - 1)); cy = fminf(fmaxf(cy, 0.0f), (float)(h - 1));
    const float fx = floorf(cx), fy = floorf(cy), ax = cx - fx, ay = cy - fy, na = 1.0f - ax, nb = 1.0f - ay;
    const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float *p00 = U + ((size_t)y0 * w + x0) * 2, *p01 = U + ((size_t)y0 * w + x1) * 2, *p10 = U + ((size_t)y1 * w + x0) * 2, *p11 = U + ((size_t)y1 * w + x1) * 2;
    const float w00 = na * nb, w01 = ax * nb, w10 = na * ay, w11 = ax * ay;
    vx = (((w00 * p00[0]) + (w01 * p01[0])) + (w10 * p10[0])) + (w11 * p11[0]);
    vy = (((w00 * p00[1]) + (w01 * p01[1])) + (w10 * p10[1])) + (w11 * p11[1]);
}

// Level `level` from the level below it, all frames: out(x, y) = (the 2 x 2 block at (2x, 2y) + 2) >> 2.  A lane per pixel.
__global__ __launch_bounds__(256) void gfw_dis_pyramid_kernel(const GfwDisLevel src, uint8_t *dst, int dw, int dh) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x);
    if (idx >= dw * dh) return;
    const int x = idx % dw, y = idx / dw;
    const uint8_t *r0 = src.base + (size_t)blockIdx.y * (size_t)src.frame_bytes + (size_t)(2 * y) * (size_t)src.stride + (size_t)(2 * x), *r1 = r0 + src.stride;
    dst[(size_t)blockIdx.y * (size_t)dw * (size_t)dh + (size_t)idx] = (uint8_t)(((int)r0[0] + (int)r0[1] + (int)r1[0] + (int)r1[1] + 2) >> 2);
}

// The exact sum of every lane's K partials: reduction r of a workgroup adds into s_acc[r % 3], lane 0 clears s_acc[(r + 1) % 3] ahead of the barrier — that one was
// last read after barrier r - 2 by lanes that have since passed barrier r - 1, and is next added to after barrier r.  One barrier a reduction.
template <int K>
__device__ __forceinline__ void gfw_dis_reduce(unsigned long long (*s_acc)[5], int &ring, int lane, const int *part, long long *sum) {
    unsigned long long *cur = s_acc[ring];
    ring = ring == 2 ? 0 : ring + 1;
    #pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(&cur[k], (unsigned long long)(long long)part[k]);
    if (lane < 5) s_acc[ring][lane] = 0ull;
    __syncthreads();
    #pragma unroll
    for (int k = 0; k < K; ++k) sum[k] = (long long)cur[k];
}

// What a wave holds of its patch, and the evaluation of a value u against the second frame: 64 times the mean-normalised SSD and the right-hand side
struct GfwDisPatch { const uint8_t *b; int w, h, stride, x, y, a32, ix, iy; long long sx, sy; };
__device__ __forceinline__ void gfw_dis_evaluate(const GfwDisPatch &P, unsigned long long (*s_acc)[5], int &ring, int lane, float ux, float uy, float &ssd, float &bx, float &by) {
    const int d = gfw_image_sample(P.b, P.w, P.h, P.stride, P.x, P.y, ux, uy) - P.a32;
    const int part[4] = {d, d * d, P.ix * d, P.iy * d};
    long long S[4];
    gfw_dis_reduce<4>(s_acc, ring, lane, part, S);
    ssd = (float)(64 * S[1] - S[0] * S[0]);
    bx = (float)(64 * S[2] - P.sx * S[0]);
    by = (float)(64 * S[3] - P.sy * S[0]);
}

// One pass of the inverse search at level `l`: workgroup (blockIdx.x, blockIdx.y) = (patch, pair), one wave.  Pass 0 descends from the start value, pass 1 from the
// patch's pass-0 value after trying its left and top neighbours' pass-0 values, pass 2 from its pass-1 value after the right and bottom neighbours' pass-1 values.
__global__ __launch_bounds__(64) void gfw_dis_pass_kernel(const GfwDisArgs A, int l, int pass) {
    __shared__ unsigned long long s_acc[3][5];
    const int pair = (int)blockIdx.y, patch = (int)blockIdx.x, lane = (int)threadIdx.x;
    const GfwDisLevel &LV = A.lv[l];
    const int w = LV.w, h = LV.h, ls = LV.stride;
    const int nx = (w - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1, ny = (h - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1;
    const int pi = patch % nx, pj = patch / nx;
    const uint8_t *la = LV.base + (size_t)A.pair_frames[pair * 2] * (size_t)LV.frame_bytes;
    GfwDisPatch P;
    P.b = LV.base + (size_t)A.pair_frames[pair * 2 + 1] * (size_t)LV.frame_bytes;
    P.w = w; P.h = h; P.stride = ls;
    P.x = GFW_DIS_STRIDE * pi + (lane & 7); P.y = GFW_DIS_STRIDE * pj + (lane >> 3);
    const uint8_t *row = la + (size_t)P.y * (size_t)ls;
    P.a32 = 32 * (int)row[P.x];
    P.ix = (int)row[min(P.x + 1, w - 1)] - (int)row[max(P.x - 1, 0)];
    P.iy = (int)la[(size_t)min(P.y + 1, h - 1) * (size_t)ls + P.x] - (int)la[(size_t)max(P.y - 1, 0) * (size_t)ls + P.x];
    if (lane < 15) s_acc[lane / 5][lane % 5] = 0ull;
    __syncthreads();
    int ring = 0;
    const int part[5] = {P.ix, P.iy, P.ix * P.ix, P.ix * P.iy, P.iy * P.iy};
    long long S[5];
    gfw_dis_reduce<5>(s_acc, ring, lane, part, S);
    P.sx = S[0]; P.sy = S[1];
    const float hxx = (float)(64 * S[2] - S[0] * S[0]), hxy = (float)(64 * S[3] - S[0] * S[1]), hyy = (float)(64 * S[4] - S[1] * S[1]);
    const float det = (hxx * hyy) - (hxy * hxy);
    // the start value: the coarser level's field at the patch centre
    float u0x = 0.0f, u0y = 0.0f;
    if (l < A.coarsest) {
        const int cw = A.lv[l + 1].w, ch = A.lv[l + 1].h;
        gfw_dis_bilinear(A.dense[l + 1] + (size_t)pair * (size_t)cw * (size_t)ch * 2, cw, ch, ((float)(GFW_DIS_STRIDE * pi + 4) * 0.5f) - 0.25f,
                         ((float)(GFW_DIS_STRIDE * pj + 4) * 0.5f) - 0.25f, u0x, u0y);
        u0x = 2.0f * u0x; u0y = 2.0f * u0y;
    }
    const size_t first = (size_t)pair * (size_t)nx * (size_t)ny;
    float *out = A.patch[pass] + (first + (size_t)patch) * 2;
    if (!(det > GFW_DIS_DET_MIN)) {                                                  // workgroup-uniform, like every branch below: never descended
        if (lane == 0) { out[0] = u0x; out[1] = u0y; }
        return;
    }
    float ux = u0x, uy = u0y, ssd, bx, by;
    const float *in = pass ? A.patch[pass - 1] + first * 2 : nullptr;
    if (pass) { ux = in[(size_t)patch * 2]; uy = in[(size_t)patch * 2 + 1]; }
    gfw_dis_evaluate(P, s_acc, ring, lane, ux, uy, ssd, bx, by);
    if (pass) {
        #pragma unroll 1
        for (int k = 0; k < 2; ++k) {
            const int ni = pi + (k == 0 ? (pass == 1 ? -1 : 1) : 0), nj = pj + (k == 1 ? (pass == 1 ? -1 : 1) : 0);
            if (ni < 0 || ni >= nx || nj < 0 || nj >= ny) continue;
            const float cx = in[((size_t)nj * nx + ni) * 2], cy = in[((size_t)nj * nx + ni) * 2 + 1];
            float s2, bx2, by2;
            gfw_dis_evaluate(P, s_acc, ring, lane, cx, cy, s2, bx2, by2);
            if (s2 < ssd) { ux = cx; uy = cy; ssd = s2; bx = bx2; by = by2; }
        }
    }
    const float idet = 1.0f / det;
    #pragma unroll 1
    for (int it = 0; it < GFW_DIS_ITERS; ++it) {
        const float dx = ((hyy * bx) - (hxy * by)) * idet, dy = ((hxx * by) - (hxy * bx)) * idet;
        const float px = ux - (0.03125f * dx), py = uy - (0.03125f * dy);
        float s2, bx2, by2;
        gfw_dis_evaluate(P, s_acc, ring, lane, px, py, s2, bx2, by2);
        if (!(s2 < ssd)) break;
        ux = px; uy = py; ssd = s2; bx = bx2; by = by2;
    }
    const float ex = ux - u0x, ey = uy - u0y;
    if (((ex * ex) + (ey * ey)) > GFW_DIS_FAR2) { ux = u0x; uy = u0y; }
    if (lane == 0) { out[0] = ux; out[1] = uy; }
}

// The dense field of level `l` from the pass-2 values: a lane per pixel, the at most four patches that cover it in row-major patch order
__global__ __launch_bounds__(256) void gfw_dis_dense_kernel(const GfwDisArgs A, int l) {
    const GfwDisLevel &LV = A.lv[l];
    const int w = LV.w, h = LV.h, ls = LV.stride;
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x), pair = (int)blockIdx.y;
    if (idx >= w * h) return;
    const int nx = (w - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1, ny = (h - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1;
    const int xc = min(idx % w, GFW_DIS_STRIDE * (nx - 1) + 7), yc = min(idx / w, GFW_DIS_STRIDE * (ny - 1) + 7);
    const uint8_t *la = LV.base + (size_t)A.pair_frames[pair * 2] * (size_t)LV.frame_bytes, *lb = LV.base + (size_t)A.pair_frames[pair * 2 + 1] * (size_t)LV.frame_bytes;
    const int a32 = 32 * (int)la[(size_t)yc * (size_t)ls + xc];
    const float *u = A.patch[2] + (size_t)pair * (size_t)nx * (size_t)ny * 2;
    const int ilo = max(0, (xc - 4) >> 2), ihi = min(xc >> 2, nx - 1), jlo = max(0, (yc - 4) >> 2), jhi = min(yc >> 2, ny - 1);
    float sw = 0.0f, sx = 0.0f, sy = 0.0f;
    for (int j = jlo; j <= jhi; ++j) {
        for (int i = ilo; i <= ihi; ++i) {
            const float ux = u[((size_t)j * nx + i) * 2], uy = u[((size_t)j * nx + i) * 2 + 1];
            const int d = gfw_image_sample(lb, w, h, ls, xc, yc, ux, uy) - a32;
            const float wt = 32.0f / (float)max(32, d < 0 ? -d : d);
            sw = sw + wt; sx = sx + (wt * ux); sy = sy + (wt * uy);
        }
    }
    float *o = A.dense[l] + ((size_t)pair * (size_t)w * (size_t)h + (size_t)idx) * 2;
    o[0] = sx / sw; o[1] = sy / sw;
}

// out_pair_first from the grid counts of the pairs' first frames: one workgroup (gfw_image_scan)
__global__ __launch_bounds__(256) void gfw_dis_scan_kernel(const GfwDisArgs A) {
    gfw_image_scan(A.n_pairs, A.out_pair_first, [&A](int p) { return A.grid_counts[A.pair_frames[p * 2]]; });
}

// The kept nodes of pair blockIdx.x's first frame through the finest field: every one is returned, in grid order
__global__ __launch_bounds__(64) void gfw_dis_nodes_kernel(const GfwDisArgs A) {
    const int pair = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int fa = A.pair_frames[pair * 2], n = A.grid_counts[fa];
    const float *node = A.grid_points + (size_t)fa * (size_t)A.grid_nodes * 2;
    const int w = A.lv[A.finest].w, h = A.lv[A.finest].h;
    const float *U = A.dense[A.finest] + (size_t)pair * (size_t)w * (size_t)h * 2;
    const float inv = A.finest == 1 ? 0.5f : 0.25f, scale = A.finest == 1 ? 2.0f : 4.0f;
    const size_t at = (size_t)A.out_pair_first[pair];
    for (int k = lane; k < n; k += 64) {
        const float i = node[(size_t)k * 2], j = node[(size_t)k * 2 + 1];
        float vx, vy;
        gfw_dis_bilinear(U, w, h, ((i + 0.5f) * inv) - 0.5f, ((j + 0.5f) * inv) - 0.5f, vx, vy);
        A.points_a[(at + k) * 2] = i; A.points_a[(at + k) * 2 + 1] = j;
        A.points_b[(at + k) * 2] = i + (scale * vx); A.points_b[(at + k) * 2 + 1] = j + (scale * vy);
    }
}

hipError_t gfw_launch_dis_pyramid(const GfwDisArgs &A, int level, uint8_t *dst, hipStream_t s) {
    if (level < 1 || level > A.coarsest || A.n_frames <= 0) return hipSuccess;
    const int dw = A.lv[level].w, dh = A.lv[level].h;
    hipLaunchKernelGGL(gfw_dis_pyramid_kernel, dim3((unsigned)(((size_t)dw * dh + 255) / 256), (unsigned)A.n_frames), dim3(64, 4), 0, s, A.lv[level - 1], dst, dw, dh);
    return hipGetLastError();
}
hipError_t gfw_launch_dis_pass(const GfwDisArgs &A, int level, int pass, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    const int nx = (A.lv[level].w - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1, ny = (A.lv[level].h - GFW_DIS_PATCH) / GFW_DIS_STRIDE + 1;
    hipLaunchKernelGGL(gfw_dis_pass_kernel, dim3((unsigned)(nx * ny), (unsigned)A.n_pairs), dim3(64), 0, s, A, level, pass);
    return hipGetLastError();
}
hipError_t gfw_launch_dis_dense(const GfwDisArgs &A, int level, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_dis_dense_kernel, dim3((unsigned)(((size_t)A.lv[level].w * A.lv[level].h + 255) / 256), (unsigned)A.n_pairs), dim3(64, 4), 0, s, A, level);
    return hipGetLastError();
}
hipError_t gfw_launch_dis_scan(const GfwDisArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_dis_scan_kernel, dim3(1), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_dis_nodes(const GfwDisArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_dis_nodes_kernel, dim3((unsigned)A.n_pairs), dim3(64), 0, s, A);
    return hipGetLastError();
}
