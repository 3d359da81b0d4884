// gfw_corners.hip — Shi-Tomasi corner detection of a clip's frames: what `OFOpenCVPyrLK::detect_features` (src/core/synchronization/optical_flow/opencv_pyrlk.rs:25-42)
// asks of good_features_to_track(img, 200, 0.01, 10.0, no mask, blockSize 3, useHarris false, 0.04).  OpenCV's source is not part of the reference tree: the contract
// is tests/_cornerstmt.py, the published Shi-Tomasi / goodFeaturesToTrack scheme stated operation by operation.
//
// Every sum is an INTEGER: the 3 x 3 Sobel derivatives of the u8 image (|D| <= 1020) on reflect-101 indices, their products, and the 3 x 3 box sums of the PRODUCT
// maps, reflected themselves (OpenCV filters `cov`; that is not the Sobel of a reflected image: Dx Dy changes sign on the border) — each below 9 * 1020^2 < 2^24, so
// exact in int32 and in its f32 conversion.  Then e = (a + c) - sqrtf((a - c)^2 + b^2) with a = Sxx * 0.5, c = Syy * 0.5, b = Sxy, one f32 rounding per operation
// (sqrtf is correctly rounded); OpenCV's scale 1 / (12 * 255) is dropped, the selection depends only on e relative to the frame's maximum.  The pick is a maximum
// over unique 64-bit keys bits(e) << 32 | (y w + x): no order of evaluation can change it.  The device equals the statement to the bit.  (The device's key holds the
// pixel as y << 13 | x — sides are at most 8192 —, which orders the pixels of a frame exactly as y w + x does and needs no division to take apart.)
//
// gfw_corners_eig_kernel: a 64 x 16 tile of a frame per workgroup (256 lanes).  The tile's pixels with a 3-pixel halo go to LDS once (reflected where the halo
// leaves the frame), the derivatives of the tile + 2 and e of the tile + 1 follow through LDS, then each lane has e of its four pixels and their neighbours.  The
// frame's maximum leaves as ONE global atomicMax per workgroup on the bits of fmaxf(e, 0) (non-negative floats order like their bits; a negative e would win as an
// unsigned word): the lanes fold into an LDS word first.  (Deviations from a reduction in the wave by shuffles, both exact: a maximum and a count do not depend on
// their order.  The host interpreter of the test suite runs this source and has no shuffles.)  Interior lanes with e > 0 and e >= all eight neighbours append their
// key to the frame's list: the slot is a ballot rank plus one atomic add per wave.  The list has room for EVERY interior pixel, and a pixel is appended at most
// once: no overflow path exists.  Its order is arbitrary and does not matter.
//
// gfw_corners_pick_kernel: a workgroup per frame runs the arg-max rounds: each round is one pass over the frame's keys that kills those within reach of the last
// accepted corner (itself included) and reduces the 64-bit maximum of the others (a lane's own first, sixteen loads in flight at a time, then one 64-bit LDS atomicMax a lane); the round's best is
// accepted if its e > t = max(e, 0) * quality, else the pick ends.  At most max_corners rounds of ceil(candidates / 256) steps a lane.
//
// NO INDEX OUTSIDE A FRAME CAN BE FORMED: a pixel is fetched only for coordinates in [-1, n] and sides are n >= 3, so one reflection (gfw_image_reflect, gfw_image.h: -1 -> 1, n -> n - 2) lands in
// [0, n - 1]; the row padding (stride > w) is never read.  Plain C++ under -ffp-contract=off; all stores are ordinary vector stores; control flow around the barriers
// is workgroup-uniform, around the ballots wave-uniform.
#include <hip/hip_runtime.h>
#include "gfw_corners.h"
#include "gfw_image.h"

#define GFW_CORNERS_PW (GFW_CORNERS_TILE_W + 6)      // pixels: the tile and a halo of 3
#define GFW_CORNERS_PH (GFW_CORNERS_TILE_H + 6)
#define GFW_CORNERS_DW (GFW_CORNERS_TILE_W + 4)      // derivatives: a halo of 2
#define GFW_CORNERS_DH (GFW_CORNERS_TILE_H + 4)
#define GFW_CORNERS_EW (GFW_CORNERS_TILE_W + 2)      // e: a halo of 1
#define GFW_CORNERS_EH (GFW_CORNERS_TILE_H + 2)
#define GFW_CORNERS_LANE_PIXELS ((GFW_CORNERS_PH * GFW_CORNERS_PW + 255) / 256)      // pixels of the haloed tile a lane fetches: 7
#define GFW_CORNERS_PICK_LOADS 16                    // keys a lane fetches before it tests them (the pick is bound by the latency of its loads)

struct GfwCornersD { int16_t x, y; };                // (Dx, Dy), |D| <= 1020

__device__ __forceinline__ unsigned gfw_corners_bits(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float gfw_corners_float(unsigned v) { return __builtin_bit_cast(float, v); }

// Workgroup (blockIdx.x, blockIdx.y) = (tile, frame of the batch)
__global__ __launch_bounds__(256) void gfw_corners_eig_kernel(const GfwCornersArgs A) {
    __shared__ uint8_t s_px[GFW_CORNERS_PH][GFW_CORNERS_PW + 2];
    __shared__ GfwCornersD s_d[GFW_CORNERS_DH][GFW_CORNERS_DW];
    __shared__ float s_e[GFW_CORNERS_EH][GFW_CORNERS_EW];
    __shared__ unsigned s_max, s_base[4];
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int frame = A.frame0 + (int)blockIdx.y;
    const int tx0 = ((int)blockIdx.x % A.tiles_x) * GFW_CORNERS_TILE_W, ty0 = ((int)blockIdx.x / A.tiles_x) * GFW_CORNERS_TILE_H;
    const int w = A.w, h = A.h;
    const uint8_t *img = A.frames + (size_t)frame * (size_t)A.frame_bytes;
    if (t == 0) s_max = 0u;
    // the pixels at (tx0 - 3 + c, ty0 - 3 + r), reflected; beyond [-1, n] nothing is ever asked: those slots hold the pixel at the clamped coordinate
    // (a lane's seven loads are issued together, then stored: one wait for the memory instead of seven)
    uint8_t px[GFW_CORNERS_LANE_PIXELS];
    #pragma unroll
    for (int u = 0; u < GFW_CORNERS_LANE_PIXELS; ++u) {
        const int i = t + 256 * u, r = i / GFW_CORNERS_PW, c = i - r * GFW_CORNERS_PW;
        const int gx = min(max(tx0 - 3 + c, -1), w), gy = min(max(ty0 - 3 + r, -1), h);      // clamped, not tested: a load without a branch, and what lies beyond is never asked
        px[u] = img[(size_t)gfw_image_reflect(gy, h) * (size_t)A.stride + (size_t)gfw_image_reflect(gx, w)];
    }
    #pragma unroll
    for (int u = 0; u < GFW_CORNERS_LANE_PIXELS; ++u) {
        const int i = t + 256 * u, r = i / GFW_CORNERS_PW, c = i - r * GFW_CORNERS_PW;
        if (i < GFW_CORNERS_PH * GFW_CORNERS_PW) s_px[r][c] = px[u];
    }
    __syncthreads();
    // the derivatives at (tx0 - 2 + c, ty0 - 2 + r) inside the frame
    for (int i = t; i < GFW_CORNERS_DH * GFW_CORNERS_DW; i += 256) {
        const int r = i / GFW_CORNERS_DW, c = i - r * GFW_CORNERS_DW;
        const int gx = tx0 - 2 + c, gy = ty0 - 2 + r;
        GfwCornersD D = {0, 0};
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const uint8_t *p0 = &s_px[r][c], *p1 = &s_px[r + 1][c], *p2 = &s_px[r + 2][c];           // rows y - 1, y, y + 1 from column x - 1
            D.x = (int16_t)(((int)p0[2] - (int)p0[0]) + 2 * ((int)p1[2] - (int)p1[0]) + ((int)p2[2] - (int)p2[0]));
            D.y = (int16_t)(((int)p2[0] - (int)p0[0]) + 2 * ((int)p2[1] - (int)p0[1]) + ((int)p2[2] - (int)p0[2]));
        }
        s_d[r][c] = D;
    }
    __syncthreads();
    // e at (tx0 - 1 + c, ty0 - 1 + r) inside the frame: the box sums of the products at reflected positions of the product maps
    for (int i = t; i < GFW_CORNERS_EH * GFW_CORNERS_EW; i += 256) {
        const int r = i / GFW_CORNERS_EW, c = i - r * GFW_CORNERS_EW;
        const int gx = tx0 - 1 + c, gy = ty0 - 1 + r;
        float e = 0.0f;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            int cx[3], sxx = 0, sxy = 0, syy = 0;
            #pragma unroll
            for (int k = 0; k < 3; ++k) cx[k] = gfw_image_reflect(gx + k - 1, w) - (tx0 - 2);
            #pragma unroll
            for (int j = 0; j < 3; ++j) {
                const GfwCornersD *row = s_d[gfw_image_reflect(gy + j - 1, h) - (ty0 - 2)];
                #pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const GfwCornersD D = row[cx[k]];
                    sxx += (int)D.x * (int)D.x; sxy += (int)D.x * (int)D.y; syy += (int)D.y * (int)D.y;
                }
            }
            const float a = (float)sxx * 0.5f, cc = (float)syy * 0.5f, b = (float)sxy;
            const float d = a - cc;
            e = (a + cc) - sqrtf((d * d) + (b * b));
        }
        s_e[r][c] = e;
    }
    __syncthreads();
    // a lane's four pixels: (tx0 + lane, ty0 + 4 m + wave)
    const int lx = (int)threadIdx.x, gx = tx0 + lx;
    unsigned long long key[4];
    int rank[4], total = 0;
    unsigned best = 0u;
    #pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int ly = 4 * m + (int)threadIdx.y, gy = ty0 + ly;
        const float e = s_e[ly + 1][lx + 1];
        const bool inside = gx < w && gy < h;
        if (inside) { const unsigned b = gfw_corners_bits(fmaxf(e, 0.0f)); best = b > best ? b : best; }
        const float *r0 = &s_e[ly][lx], *r1 = &s_e[ly + 1][lx], *r2 = &s_e[ly + 2][lx];      // (every lane's nine lie inside s_e; & for &&: no branches)
        const bool cand = (gx >= 1) & (gx <= w - 2) & (gy >= 1) & (gy <= h - 2) & (e > 0.0f) &
                          (e >= r0[0]) & (e >= r0[1]) & (e >= r0[2]) & (e >= r1[0]) & (e >= r1[2]) & (e >= r2[0]) & (e >= r2[1]) & (e >= r2[2]);
        key[m] = ((unsigned long long)gfw_corners_bits(e) << 32) | (unsigned long long)(((unsigned)gy << 13) | (unsigned)gx);
        const unsigned long long mask = __ballot(cand);
        rank[m] = cand ? total + gfw_image_ballot_rank(mask) : -1;
        total += (int)__popcll(mask);
    }
    if (best) atomicMax(&s_max, best);
    if (lx == 0 && total) s_base[threadIdx.y] = atomicAdd(&A.cand_count[frame], (unsigned)total);
    __syncthreads();
    if (t == 0 && s_max) atomicMax(&A.max_bits[frame], s_max);
    if (total) {
        unsigned long long *list = A.cand + (size_t)blockIdx.y * (size_t)A.slots + (size_t)s_base[threadIdx.y];
        #pragma unroll
        for (int m = 0; m < 4; ++m) if (rank[m] >= 0) list[rank[m]] = key[m];
    }
}

// Workgroup blockIdx.x = a frame of the batch.  Reduction r adds into s_best[r % 3], lane 0 clears s_best[(r + 1) % 3] ahead of the barrier: that one was last read
// after barrier r - 2 by lanes that have since passed barrier r - 1, and is next added to after barrier r.  One barrier a round.
__global__ __launch_bounds__(256) void gfw_corners_pick_kernel(const GfwCornersArgs A) {
    __shared__ unsigned long long s_best[3];
    const int t = (int)(threadIdx.y * 64u + threadIdx.x);
    const int frame = A.frame0 + (int)blockIdx.x;
    const int n = (int)A.cand_count[frame];
    unsigned long long *keys = A.cand + (size_t)blockIdx.x * (size_t)A.slots;
    const float thr = gfw_corners_float(A.max_bits[frame]) * A.quality;
    const float reach = A.min_distance * A.min_distance;
    float *corners = A.corners + (size_t)frame * (size_t)A.max_corners * 2;
    float *scores = A.scores ? A.scores + (size_t)frame * (size_t)A.max_corners : nullptr;
    if (t < 3) s_best[t] = 0ull;
    __syncthreads();
    int ring = 0, count = 0, last_x = 0, last_y = 0;
    unsigned last = 0xFFFFFFFFu;                                                     // the pixel index of the last accepted corner; none yet
    #pragma unroll 1
    for (int round = 0; round < A.max_corners; ++round) {                            // workgroup-uniform, like the exits below
        unsigned long long *cur = &s_best[ring];
        ring = ring == 2 ? 0 : ring + 1;
        unsigned long long best = 0ull;
        for (int base = t; base < n; base += 256 * GFW_CORNERS_PICK_LOADS) {         // a lane's keys: t + 256 j; sixteen loads in flight, then their tests
            unsigned long long k[GFW_CORNERS_PICK_LOADS];
            #pragma unroll
            for (int u = 0; u < GFW_CORNERS_PICK_LOADS; ++u) { const int i = base + 256 * u; k[u] = i < n ? keys[i] : 0ull; }
            #pragma unroll
            for (int u = 0; u < GFW_CORNERS_PICK_LOADS; ++u) {
                if (k[u] == 0ull) continue;
                if (last != 0xFFFFFFFFu) {
                    const unsigned idx = (unsigned)k[u];
                    const int dx = (int)(idx & 8191u) - last_x, dy = (int)(idx >> 13) - last_y;
                    if (idx == last || (float)(dx * dx + dy * dy) < reach) { keys[base + 256 * u] = 0ull; continue; }
                }
                best = k[u] > best ? k[u] : best;
            }
        }
        if (best) atomicMax(cur, best);
        if (t == 0) s_best[ring] = 0ull;
        __syncthreads();
        const unsigned long long top = *cur;
        const float e = gfw_corners_float((unsigned)(top >> 32));
        if (top == 0ull || !(e > thr)) break;
        last = (unsigned)top;
        last_y = (int)(last >> 13); last_x = (int)(last & 8191u);
        if (t == 0) {
            corners[(size_t)count * 2] = (float)last_x; corners[(size_t)count * 2 + 1] = (float)last_y;
            if (scores) scores[count] = e;
        }
        ++count;
    }
    for (int k = count + t; k < A.max_corners; k += 256) {
        corners[(size_t)k * 2] = 0.0f; corners[(size_t)k * 2 + 1] = 0.0f;
        if (scores) scores[k] = 0.0f;
    }
    if (t == 0) A.counts[frame] = count;
}

// feat_first from the frames' counts: one workgroup (gfw_image_scan)
__global__ __launch_bounds__(256) void gfw_corners_scan_kernel(const GfwCornersArgs A) {
    gfw_image_scan(A.n_frames, A.feat_first, [&A](int f) { return A.counts[f]; });
}

// The corners of frame blockIdx.x in pick order behind those of the frames before it
__global__ __launch_bounds__(64) void gfw_corners_pack_kernel(const GfwCornersArgs A) {
    const int frame = (int)blockIdx.x, lane = (int)threadIdx.x;
    const float *corners = A.corners + (size_t)frame * (size_t)A.max_corners * 2;
    float *out = A.features + (size_t)A.feat_first[frame] * 2;
    const int n = A.counts[frame];
    for (int k = lane; k < n; k += 64) { out[(size_t)k * 2] = corners[(size_t)k * 2]; out[(size_t)k * 2 + 1] = corners[(size_t)k * 2 + 1]; }
}

hipError_t gfw_launch_corners_eig(const GfwCornersArgs &A, hipStream_t s) {
    if (A.batch_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_corners_eig_kernel, dim3((unsigned)(A.tiles_x * A.tiles_y), (unsigned)A.batch_frames), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_corners_pick(const GfwCornersArgs &A, hipStream_t s) {
    if (A.batch_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_corners_pick_kernel, dim3((unsigned)A.batch_frames), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_corners_scan(const GfwCornersArgs &A, hipStream_t s) {
    if (A.n_frames <= 0 || !A.feat_first) return hipSuccess;
    hipLaunchKernelGGL(gfw_corners_scan_kernel, dim3(1), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_corners_pack(const GfwCornersArgs &A, hipStream_t s) {
    if (A.n_frames <= 0 || !A.feat_first) return hipSuccess;
    hipLaunchKernelGGL(gfw_corners_pack_kernel, dim3((unsigned)A.n_frames), dim3(64), 0, s, A);
    return hipGetLastError();
}
