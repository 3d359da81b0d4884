// gfw_flow.hip — pyramidal Lucas-Kanade optical flow of a clip's frame pairs: the given features of each pair's first frame tracked into its second frame, what
// `OFOpenCVPyrLK::optical_flow_to` (src/core/synchronization/optical_flow/opencv_pyrlk.rs:63-119) asks of calcOpticalFlowPyrLK with window 21 x 21, maxLevel 3,
// 30 iterations or eps 0.01, flags 0 and minEigThreshold 1e-4, and its filter of the result (:88-100).  OpenCV's source is not part of the reference tree: the
// contract is tests/_flowstmt.py, the published pyramidal Lucas-Kanade scheme stated operation by operation.
//
// Every window sum is an INTEGER: pixels, Scharr derivatives and bilinear samples are fixed point (gfw_image.h's weights of 14 bits that sum to 16384), the products of a window
// are summed exactly (a lane's seven fit an int32 — 7 * 8160 * 4080 < 2^31 —, the 441 of a window need an int64: 441 * 4080^2 > 2^32), and one conversion to f32
// follows each reduction.  The order of an exact sum is free, so the wave reduces with 64-bit LDS atomics and the result equals the statement's to the bit.
//
// A workgroup is ONE wave per (pair, feature): a barrier is a wave barrier.  The wave keeps the template's 441 (I, Ix, Iy) in registers, seven window pixels a lane,
// and walks the levels and iterations itself; every lane computes the same f32 update from the same sums, so the trip counts are wave-uniform by construction.
// J is fetched by four byte gathers per window pixel straight from the level (a level of a 1280 x 720 clip's frame is at most 0.9 MB: L2-resident; the alternative,
// the 22 x 22 patch staged through LDS once per iteration, costs a barrier more per iteration and was not measured against this).
//
// NO INDEX OUTSIDE A LEVEL CAN BE FORMED.  A level has sides n >= 24 (GFW_FLOW_SIDE_MIN: the host builds no smaller one).  The iteration reads B at columns
// iv .. iv + 21 (21 window pixels and the bilinear neighbour) and is entered only with -21 <= iv <= n - 1 (tested on the float BEFORE the cast, which is only made
// for |g| < 2^24), so its indices lie in [-21, n + 20].  The template reads A at iu - 1 .. iu + 22 (the Scharr taps of both bilinear neighbours) with
// iu = floor(p * 2^-l - 10) for a feature 0 <= p < w, so -10 <= iu <= n - 10 and its indices lie in [-11, n + 12].  gfw_image_reflect (gfw_image.h) maps i < 0 to -i <= 22 <= n - 1
// and i >= n to 2n - 2 - i >= 2n - 2 - (n + 21) = n - 23 >= 0: one reflection lands inside [0, n - 1] for every index in [-22, n + 21] when n >= 23, and the cut at
// 24 leaves one to spare.  The pyramid reads 2x - 2 .. 2x + 2 with x <= (n + 1) / 2 - 1: indices in [-2, n + 1], inside by the same map.  Rows alike.
// Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; control flow around the barriers is workgroup-uniform, around the ballots wave-uniform.
#include <hip/hip_runtime.h>
#include "gfw_flow.h"
#include "gfw_image.h"

#define GFW_FLOW_EPSILON 1.1920928955078125e-7f      // FLT_EPSILON

__device__ __forceinline__ bool gfw_flow_inside(float x, float y, float w, float h) { return x >= 0.0f && x < w && y >= 0.0f && y < h; }      // false for a NaN

// Level `level` from the level below it, all frames: out(x, y) = (sum k_i k_j in(r(2x + i), r(2y + j)) + 128) >> 8, k = 1 4 6 4 1.  A lane per pixel.
__global__ __launch_bounds__(256) void gfw_flow_pyramid_kernel(const GfwFlowLevel src, uint8_t *dst, int dw, int dh) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x);
    if (idx >= dw * dh) return;
    const int x = idx % dw, y = idx / dw;
    const uint8_t *in = src.base + (size_t)blockIdx.y * (size_t)src.frame_bytes;
    int xs[5];
    #pragma unroll
    for (int i = 0; i < 5; ++i) xs[i] = gfw_image_reflect(2 * x + i - 2, src.w);
    int acc = 0;
    #pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t *row = in + (size_t)gfw_image_reflect(2 * y + j - 2, src.h) * (size_t)src.stride;
        const int r = (int)row[xs[0]] + 4 * (int)row[xs[1]] + 6 * (int)row[xs[2]] + 4 * (int)row[xs[3]] + (int)row[xs[4]];
        acc += (j == 0 || j == 4 ? 1 : (j == 2 ? 6 : 4)) * r;
    }
    dst[(size_t)blockIdx.y * (size_t)dw * (size_t)dh + (size_t)idx] = (uint8_t)((acc + 128) >> 8);
}

// The grid points of frame blockIdx.x (opencv_dis.rs:62-119): node k is (i, j) = ((k / rows) * step, (k % rows) * step), `i` the outer loop.  A lane folds its
// node's window in the reference's order (ny outer, nx inner, sequential f32), the wave ranks the kept nodes by ballot: node order is the reference's push order.
__global__ __launch_bounds__(64) void gfw_flow_grid_kernel(const GfwFlowArgs A) {
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const GfwFlowLevel &L0 = A.lv[0];
    const uint8_t *img = L0.base + (size_t)f * (size_t)L0.frame_bytes;
    float *out = A.grid_points + (size_t)f * (size_t)A.grid_nodes * 2;
    int packed = 0;
    for (int base = 0; base < A.grid_nodes; base += 64) {                            // wave-uniform
        const int k = base + lane;
        bool keep = false;
        int i = 0, j = 0;
        if (k < A.grid_nodes) {
            i = (k / A.grid_rows) * A.grid_step; j = (k % A.grid_rows) * A.grid_step;
            const int y0 = max(j - A.grid_half, 0), y1 = min(j + A.grid_half, L0.h - 1), x0 = max(i - A.grid_half, 0), x1 = min(i + A.grid_half, L0.w - 1);
            float sum = 0.0f, sum_sq = 0.0f, count = 0.0f;
            for (int ny = y0; ny <= y1; ++ny) {
                const uint8_t *row = img + (size_t)ny * (size_t)L0.stride;
                for (int nx = x0; nx <= x1; ++nx) {
                    const float pixel = (float)row[nx];
                    sum = sum + pixel;
                    sum_sq = sum_sq + (pixel * pixel);
                    count = count + 1.0f;
                }
            }
            const float mean = sum / count;
            keep = ((sum_sq / count) - (mean * mean)) > 3.0f;
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int at = packed + gfw_image_ballot_rank(mask);
            out[(size_t)at * 2] = (float)i; out[(size_t)at * 2 + 1] = (float)j;
        }
        packed += (int)__popcll(mask);
    }
    for (int k = packed + lane; k < A.grid_nodes; k += 64) { out[(size_t)k * 2] = 0.0f; out[(size_t)k * 2 + 1] = 0.0f; }
    if (lane == 0) A.grid_counts[f] = packed;
}

// The features of a pair's first frame: -> the list, its length `n`, and the raw slots the pair has (`n`, or every node of the grid)
__device__ __forceinline__ const float *gfw_flow_features(const GfwFlowArgs &A, int frame, int &n, int &slots) {
    if (A.mode == GFW_FLOW_MODE_GRID) { n = A.grid_counts[frame]; slots = A.grid_nodes; return A.grid_points + (size_t)frame * (size_t)A.grid_nodes * 2; }
    const int first = A.feat_first[frame];
    n = A.feat_first[frame + 1] - first; slots = n;
    return A.features + (size_t)first * 2;
}

// The exact sum of every lane's K partials: reduction r of a workgroup adds into s_acc[r % 3], lane 0 clears s_acc[(r + 1) % 3] ahead of the barrier — that one was
// last read after barrier r - 2 by lanes that have since passed barrier r - 1, and is next added to after barrier r.  One barrier a reduction.
template <int K>
__device__ __forceinline__ void gfw_flow_reduce(unsigned long long (*s_acc)[3], int &ring, int lane, const int *part, long long *sum) {
    unsigned long long *cur = s_acc[ring];
    ring = ring == 2 ? 0 : ring + 1;
    #pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(&cur[k], (unsigned long long)(long long)part[k]);
    if (lane == 0) { s_acc[ring][0] = 0ull; s_acc[ring][1] = 0ull; s_acc[ring][2] = 0ull; }
    __syncthreads();
    #pragma unroll
    for (int k = 0; k < K; ++k) sum[k] = (long long)cur[k];
}

// The tracker: workgroup (blockIdx.x, blockIdx.y) = (feature, pair), one wave
__global__ __launch_bounds__(64) void gfw_flow_track_kernel(const GfwFlowArgs A) {
    __shared__ unsigned long long s_acc[3][3];
    const int pair = (int)blockIdx.y, k = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int fa = A.pair_frames[pair * 2], fb = A.pair_frames[pair * 2 + 1];
    int n, slots;
    const float *feat = gfw_flow_features(A, fa, n, slots);
    if (k >= slots) return;                                                          // workgroup-uniform, like every branch below
    const size_t raw = (size_t)A.raw_first[pair] + (size_t)k;
    const float width = (float)A.lv[0].w, height = (float)A.lv[0].h;
    float fx = 0.0f, fy = 0.0f;
    if (k < n) { fx = feat[(size_t)k * 2]; fy = feat[(size_t)k * 2 + 1]; }
    if (lane == 0 && A.iters) { int32_t *o = A.iters + raw * 4; o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; }
    if (!(k < n && gfw_flow_inside(fx, fy, width, height))) {                        // not tracked: a non-finite feature, one outside the frame, an unused grid slot
        if (lane == 0) { A.next[raw * 2] = fx; A.next[raw * 2 + 1] = fy; A.status[raw] = 0; }
        return;
    }
    if (lane < 9) s_acc[lane / 3][lane % 3] = 0ull;
    __syncthreads();
    int ring = 0, status = 1;
    float gx = 0.0f, gy = 0.0f;
    #pragma unroll 1
    for (int l = A.top; l >= 0; --l) {
        const GfwFlowLevel &LV = A.lv[l];
        const int lw = LV.w, lh = LV.h, ls = LV.stride;
        const uint8_t *la = LV.base + (size_t)fa * (size_t)LV.frame_bytes, *lb = LV.base + (size_t)fb * (size_t)LV.frame_bytes;
        const float scale = l == 0 ? 1.0f : (l == 1 ? 0.5f : (l == 2 ? 0.25f : 0.125f));
        const float ux = (fx * scale) - 10.0f, uy = (fy * scale) - 10.0f;
        if (l == A.top) { gx = ux; gy = uy; }
        else { gx = (2.0f * (gx + 10.0f)) - 10.0f; gy = (2.0f * (gy + 10.0f)) - 10.0f; }
        // the template: I with 5 fraction bits, Ix and Iy in the Scharr derivative's own units, at floor(u) with u's weights
        const float fux = floorf(ux), fuy = floorf(uy);
        const int iux = (int)fux, iuy = (int)fuy;                                    // -10 <= iu < 8192
        const GfwImageWeights W = gfw_image_weights(ux - fux, uy - fuy);
        int I[GFW_FLOW_LANE_PIXELS], Ix[GFW_FLOW_LANE_PIXELS], Iy[GFW_FLOW_LANE_PIXELS];
        int part[3] = {0, 0, 0};
        #pragma unroll
        for (int m = 0; m < GFW_FLOW_LANE_PIXELS; ++m) {
            const int wk = lane + 64 * m;
            I[m] = 0; Ix[m] = 0; Iy[m] = 0;
            if (wk < GFW_FLOW_WIN_PIXELS) {
                const int wy = wk / GFW_FLOW_WIN, wx = wk - wy * GFW_FLOW_WIN;
                int v[4][4];
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint8_t *row = la + (size_t)gfw_image_reflect(iuy + wy - 1 + r, lh) * (size_t)ls;
                    #pragma unroll
                    for (int c = 0; c < 4; ++c) v[r][c] = (int)row[gfw_image_reflect(iux + wx - 1 + c, lw)];
                }
                int dx[2][2], dy[2][2];                                              // the derivatives at (x + c, y + r)
                #pragma unroll
                for (int r = 0; r < 2; ++r) {
                    #pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        dx[r][c] = 3 * (v[r][c + 2] - v[r][c]) + 10 * (v[r + 1][c + 2] - v[r + 1][c]) + 3 * (v[r + 2][c + 2] - v[r + 2][c]);
                        dy[r][c] = 3 * (v[r + 2][c] - v[r][c]) + 10 * (v[r + 2][c + 1] - v[r][c + 1]) + 3 * (v[r + 2][c + 2] - v[r][c + 2]);
                    }
                }
                I[m] = (W.w00 * v[1][1] + W.w01 * v[1][2] + W.w10 * v[2][1] + W.w11 * v[2][2] + 256) >> 9;
                Ix[m] = (W.w00 * dx[0][0] + W.w01 * dx[0][1] + W.w10 * dx[1][0] + W.w11 * dx[1][1] + 8192) >> 14;
                Iy[m] = (W.w00 * dy[0][0] + W.w01 * dy[0][1] + W.w10 * dy[1][0] + W.w11 * dy[1][1] + 8192) >> 14;
                part[0] += Ix[m] * Ix[m]; part[1] += Ix[m] * Iy[m]; part[2] += Iy[m] * Iy[m];
            }
        }
        long long sum[3];
        gfw_flow_reduce<3>(s_acc, ring, lane, part, sum);
        const float s = 1.0f / 1048576.0f;
        const float a11 = (float)sum[0] * s, a12 = (float)sum[1] * s, a22 = (float)sum[2] * s;
        float D = (a11 * a22) - (a12 * a12);
        const float dif = a11 - a22;
        const float min_eig = ((a22 + a11) - sqrtf((dif * dif) + ((4.0f * a12) * a12))) / 882.0f;
        if (min_eig < 1e-4f || D < GFW_FLOW_EPSILON) {                               // the level is skipped: the guess passes down unchanged
            if (l == 0) status = 0;
            continue;
        }
        D = 1.0f / D;
        float pdx = 0.0f, pdy = 0.0f;
        int count = 0;
        #pragma unroll 1
        for (int j = 0; j < GFW_FLOW_ITERS; ++j) {
            // tested before any float -> int cast: a cast outside the int range is never executed
            if (!(fabsf(gx) < 16777216.0f) || !(fabsf(gy) < 16777216.0f)) { if (l == 0) status = 0; break; }
            const float fgx = floorf(gx), fgy = floorf(gy);
            if (fgx < -21.0f || fgx >= (float)lw || fgy < -21.0f || fgy >= (float)lh) { if (l == 0) status = 0; break; }
            const int ivx = (int)fgx, ivy = (int)fgy;
            const GfwImageWeights V = gfw_image_weights(gx - fgx, gy - fgy);
            int pb[2] = {0, 0};
            #pragma unroll
            for (int m = 0; m < GFW_FLOW_LANE_PIXELS; ++m) {
                const int wk = lane + 64 * m;
                if (wk < GFW_FLOW_WIN_PIXELS) {
                    const int wy = wk / GFW_FLOW_WIN, wx = wk - wy * GFW_FLOW_WIN;
                    const uint8_t *r0 = lb + (size_t)gfw_image_reflect(ivy + wy, lh) * (size_t)ls, *r1 = lb + (size_t)gfw_image_reflect(ivy + wy + 1, lh) * (size_t)ls;
                    const int c0 = gfw_image_reflect(ivx + wx, lw), c1 = gfw_image_reflect(ivx + wx + 1, lw);
                    const int J = (V.w00 * (int)r0[c0] + V.w01 * (int)r0[c1] + V.w10 * (int)r1[c0] + V.w11 * (int)r1[c1] + 256) >> 9;
                    const int d = J - I[m];
                    pb[0] += d * Ix[m]; pb[1] += d * Iy[m];
                }
            }
            long long B[2];
            gfw_flow_reduce<2>(s_acc, ring, lane, pb, B);
            const float b1 = (float)B[0] * s, b2 = (float)B[1] * s;
            const float dx = ((a12 * b2) - (a22 * b1)) * D, dy = ((a12 * b1) - (a11 * b2)) * D;
            gx = gx + dx; gy = gy + dy;
            count = j + 1;
            if (((dx * dx) + (dy * dy)) <= 1e-4f) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) { gx = gx - (0.5f * dx); gy = gy - (0.5f * dy); break; }
            pdx = dx; pdy = dy;
        }
        if (lane == 0 && A.iters) A.iters[raw * 4 + l] = count;
    }
    if (lane == 0) {
        const float nx = gx + 10.0f, ny = gy + 10.0f;
        A.next[raw * 2] = nx; A.next[raw * 2 + 1] = ny; A.status[raw] = (uint8_t)status;
        if (status == 1 && gfw_flow_inside(nx, ny, width, height)) atomicAdd(&A.kept[pair], 1);      // the filter of opencv_pyrlk.rs:88-100
    }
}

// out_pair_first from the pairs' kept counts: one workgroup (gfw_image_scan)
__global__ __launch_bounds__(256) void gfw_flow_scan_kernel(const GfwFlowArgs A) {
    gfw_image_scan(A.n_pairs, A.out_pair_first, [&A](int p) { return A.kept[p]; });
}

// The kept points of pair blockIdx.x in feature order, ranked by ballot
__global__ __launch_bounds__(64) void gfw_flow_compact_kernel(const GfwFlowArgs A) {
    const int pair = (int)blockIdx.x, lane = (int)threadIdx.x;
    int n, slots;
    const float *feat = gfw_flow_features(A, A.pair_frames[pair * 2], n, slots);
    const size_t raw0 = (size_t)A.raw_first[pair];
    const float width = (float)A.lv[0].w, height = (float)A.lv[0].h;
    int at = A.out_pair_first[pair];
    for (int base = 0; base < slots; base += 64) {                                   // wave-uniform
        const int k = base + lane;
        bool keep = false;
        float nx = 0.0f, ny = 0.0f;
        if (k < slots && A.status[raw0 + k] == 1) {
            nx = A.next[(raw0 + k) * 2]; ny = A.next[(raw0 + k) * 2 + 1];
            keep = gfw_flow_inside(nx, ny, width, height);
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const size_t o = (size_t)(at + gfw_image_ballot_rank(mask)) * 2;
            A.points_a[o] = feat[(size_t)k * 2]; A.points_a[o + 1] = feat[(size_t)k * 2 + 1];
            A.points_b[o] = nx; A.points_b[o + 1] = ny;
        }
        at += (int)__popcll(mask);
    }
}

hipError_t gfw_launch_flow_pyramid(const GfwFlowArgs &A, int level, uint8_t *dst, hipStream_t s) {
    if (level < 1 || level > A.top || A.n_frames <= 0) return hipSuccess;
    const int dw = A.lv[level].w, dh = A.lv[level].h;
    hipLaunchKernelGGL(gfw_flow_pyramid_kernel, dim3((unsigned)(((size_t)dw * dh + 255) / 256), (unsigned)A.n_frames), dim3(64, 4), 0, s, A.lv[level - 1], dst, dw, dh);
    return hipGetLastError();
}
hipError_t gfw_launch_flow_grid(const GfwFlowArgs &A, hipStream_t s) {
    if (A.mode != GFW_FLOW_MODE_GRID || A.n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_flow_grid_kernel, dim3((unsigned)A.n_frames), dim3(64), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_flow_track(const GfwFlowArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0 || A.max_features <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_flow_track_kernel, dim3((unsigned)A.max_features, (unsigned)A.n_pairs), dim3(64), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_flow_scan(const GfwFlowArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_flow_scan_kernel, dim3(1), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_flow_compact(const GfwFlowArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_flow_compact_kernel, dim3((unsigned)A.n_pairs), dim3(64), 0, s, A);
    return hipGetLastError();
}
