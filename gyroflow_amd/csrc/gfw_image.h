// gfw_image.h — device helpers of the image-side sync units (gfw_flow.hip, gfw_corners.hip, gfw_dis.hip, gfw_varref.hip), stated ONCE: the index maps that keep
// every fetch inside a level, the fixed-point bilinear sampler behind the exact integer sums, a lane's rank in a ballot, and the one-workgroup exclusive scan.
// Device only, plain C++ under -ffp-contract=off: every f32 operation below is one operation, in the order of the numpy statements (tests/_flowstmt.py,
// tests/_disstmt.py, tests/_varrefstmt.py).  Each unit's head comment says for which arguments it calls these; what the functions themselves guarantee:
//   gfw_image_clamp(i, n)    lies in [0, n - 1] for EVERY int i (n >= 1);
//   gfw_image_reflect(i, n)  lies in [0, n - 1] for -(n - 1) <= i <= 2 n - 2, and only there: the callers bound i;
//   gfw_image_sample         reads only at clamped columns and rows, its integer displacement clamped to +-16384 as a FLOAT before the cast (no cast outside the
//                            int range is executed; |x + ix + 1| < 2^15 for sides <= 8192), and never the row padding (stride > w).
//
// The include guard stands beside `#pragma once` on purpose: the host interpreter of the test suite expands `#include "..."` textually, drops the pragma, and may
// join the texts of several units into one translation unit; a text that holds this header more than once must still compile.
#pragma once
#ifndef GFW_IMAGE_H
#define GFW_IMAGE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ int gfw_image_clamp(int i, int n) { return min(max(i, 0), n - 1); }
__device__ __forceinline__ int gfw_image_reflect(int i, int n) {                     // reflect-101: -1 -> 1, n -> n - 2
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// The four 14-bit weights of a position's fraction (a, b): every operation one f32 operation, rintf rounds half to even; they sum to 16384
struct GfwImageWeights { int w00, w01, w10, w11; };
__device__ __forceinline__ GfwImageWeights gfw_image_weights(float a, float b) {
    const float na = 1.0f - a, nb = 1.0f - b;
    GfwImageWeights W;
    W.w00 = (int)rintf((na * nb) * 16384.0f);
    W.w01 = (int)rintf((a * nb) * 16384.0f);
    W.w10 = (int)rintf((na * b) * 16384.0f);
    W.w11 = 16384 - W.w00 - W.w01 - W.w10;
    return W;
}
// The level `img` at the pixel (x, y) displaced by (ux, uy), edge replicated, 5 fraction bits: 0 .. 8160
__device__ __forceinline__ int gfw_image_sample(const uint8_t *img, int w, int h, int stride, int x, int y, float ux, float uy) {
    const float fx = floorf(ux), fy = floorf(uy);
    const GfwImageWeights W = gfw_image_weights(ux - fx, uy - fy);
    const int ix = (int)fminf(fmaxf(fx, -16384.0f), 16384.0f), iy = (int)fminf(fmaxf(fy, -16384.0f), 16384.0f);
    const int c0 = gfw_image_clamp(x + ix, w), c1 = gfw_image_clamp(x + ix + 1, w);
    const uint8_t *r0 = img + (size_t)gfw_image_clamp(y + iy, h) * (size_t)stride, *r1 = img + (size_t)gfw_image_clamp(y + iy + 1, h) * (size_t)stride;
    return (W.w00 * (int)r0[c0] + W.w01 * (int)r0[c1] + W.w10 * (int)r1[c0] + W.w11 * (int)r1[c1] + 256) >> 9;
}

// The number of set bits of a wave's ballot below the calling lane: its slot among the lanes that voted true
__device__ __forceinline__ int gfw_image_ballot_rank(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// first[i] = count(0) + .. + count(i - 1) for i = 0 .. n, by ONE workgroup of 256 lanes (64 x 4): lane t owns a run of consecutive items.  `count` is read twice
// per item and must not change meanwhile; first[] has n + 1 elements.  Every lane of the workgroup calls it (a barrier inside).
template <typename Count>
__device__ __forceinline__ void gfw_image_scan(int n, int *first, Count count) {
    __shared__ int s_sum[256];
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int run = (n + 255) / 256, lo = min(t * run, n), hi = min(lo + run, n);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += count(i);
    s_sum[t] = sum;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < t; ++j) before += s_sum[j];
    for (int i = lo; i < hi; ++i) { first[i] = before; before += count(i); }
    if (t == 255) first[n] = before;                                                  // lane 255's run is the last (possibly empty) one
}
#endif  // GFW_IMAGE_H
