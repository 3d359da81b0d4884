// gfw_varref.hip — variational refinement of the DIS dense flow's fields (gfw_varref.h): per level and pair, directly behind gfw_dis_dense_kernel, the field U is
// refined in place by fixed_point_iters linearisations of the Brox energy (brightness constancy, gradient constancy, smoothness), each solved by sor_iters red-black
// SOR iterations.  The contract is tests/_varrefstmt.py, operation by operation: everything is f32, every written operator is one operation (-ffp-contract=off;
// `/` and sqrtf are correctly rounded, denormals are kept), sums run left to right, the four links of a pixel always in the order right, left, down, up.  A link that
// does not exist has the weight 0 and the pixel itself as its neighbour, so a border pixel runs the very operations of an inner one.
//
// The fixed-point sampler (14-bit weights, 5 fraction bits, edge replicated) is gfw_image_sample of gfw_image.h, the one the DIS flow itself samples with; the
// clamp c below is that header's gfw_image_clamp.
//
// A lane per pixel and pair (a lane per pixel of ONE colour in the half-sweep); the pair rides on blockIdx.y.  Within a half-sweep a pixel reads du, dv of its
// four neighbours, which have the other colour and are not written by this launch, and its own: the result does not depend on the order in which lanes run.
//
// NO INDEX OUTSIDE A LEVEL CAN BE FORMED.  idx < w h gives x = idx % w < w and y = idx / w < h (the half-sweep: y = idx / ceil(w / 2) < h, and a lane whose
// x = 2 i + ((y + colour) & 1) reaches w leaves before it reads).  Every neighbour is read at c(x +- 1, w), c(y +- 1, h) with c(i, n) = min(max(i, 0), n - 1), also
// where clamps compose (the second derivatives); the smoothness term reads (x + 1, y) only under x + 1 < w and (x, y + 1) only under y + 1 < h, at positions that
// lie in the level themselves.  The sampler clamps its integer displacement to +-16384 as a float before the cast and its columns and rows into the level.  Sides
// are <= 8192 and pairs <= 65535, a level of the refinement is at most 4096 x 4096: indices are formed in size_t.  No LDS, no scratch, ordinary vector stores.
#include <hip/hip_runtime.h>
#include "gfw_varref.h"
#include "gfw_image.h"

// What the prepare kernel sees of a pair's level: avg = (I0 + I1w) 0.5 and Iz = I1w - I0 at a pixel INSIDE the level, I1w the second image warped by the field
struct GfwVarrefImages { const uint8_t *a, *b; const float *U; int w, h, stride; };
__device__ __forceinline__ void gfw_varref_warped(const GfwVarrefImages &G, int x, int y, float &avg, float &iz) {
    const float *u = G.U + ((size_t)y * (size_t)G.w + (size_t)x) * 2;
    const float i0 = (float)G.a[(size_t)y * (size_t)G.stride + (size_t)x];
    const float i1 = (float)gfw_image_sample(G.b, G.w, G.h, G.stride, x, y, u[0], u[1]) * 0.03125f;
    avg = (i0 + i1) * 0.5f; iz = i1 - i0;
}
// dx and dy of avg and Iz at a pixel inside the level: (a(c(x + 1)) - a(c(x - 1))) 0.5
__device__ __forceinline__ void gfw_varref_dx(const GfwVarrefImages &G, int x, int y, float &ix, float &izx) {
    float a1, z1, a0, z0;
    gfw_varref_warped(G, gfw_image_clamp(x + 1, G.w), y, a1, z1);
    gfw_varref_warped(G, gfw_image_clamp(x - 1, G.w), y, a0, z0);
    ix = (a1 - a0) * 0.5f; izx = (z1 - z0) * 0.5f;
}
__device__ __forceinline__ void gfw_varref_dy(const GfwVarrefImages &G, int x, int y, float &iy, float &izy) {
    float a1, z1, a0, z0;
    gfw_varref_warped(G, x, gfw_image_clamp(y + 1, G.h), a1, z1);
    gfw_varref_warped(G, x, gfw_image_clamp(y - 1, G.h), a0, z0);
    iy = (a1 - a0) * 0.5f; izy = (z1 - z0) * 0.5f;
}

// Once per level: the derivative images of every pixel from the warped image over its footprint, du = dv = 0
__global__ __launch_bounds__(256) void gfw_varref_prepare_kernel(const GfwVarrefArgs A) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x), pair = (int)blockIdx.y;
    const int w = A.w, h = A.h;
    if (idx >= w * h) return;
    const int x = idx % w, y = idx / w;
    GfwVarrefImages G;
    G.a = A.base + (size_t)A.pair_frames[pair * 2] * (size_t)A.frame_bytes; G.b = A.base + (size_t)A.pair_frames[pair * 2 + 1] * (size_t)A.frame_bytes;
    G.U = A.U + (size_t)pair * (size_t)w * (size_t)h * 2; G.w = w; G.h = h; G.stride = A.stride;
    float avg, iz, ix, iy, ixz, iyz, p, m, unused;
    gfw_varref_warped(G, x, y, avg, iz);
    gfw_varref_dx(G, x, y, ix, ixz);
    gfw_varref_dy(G, x, y, iy, iyz);
    const int xp = gfw_image_clamp(x + 1, w), xm = gfw_image_clamp(x - 1, w), yp = gfw_image_clamp(y + 1, h), ym = gfw_image_clamp(y - 1, h);
    gfw_varref_dx(G, xp, y, p, unused); gfw_varref_dx(G, xm, y, m, unused);
    const float ixx = (p - m) * 0.5f;
    gfw_varref_dx(G, x, yp, p, unused); gfw_varref_dx(G, x, ym, m, unused);
    const float ixy = (p - m) * 0.5f;
    gfw_varref_dy(G, x, yp, p, unused); gfw_varref_dy(G, x, ym, m, unused);
    const float iyy = (p - m) * 0.5f;
    const size_t at = (size_t)pair * (size_t)w * (size_t)h + (size_t)idx;
    A.plane[GFW_VR_IX][at] = ix; A.plane[GFW_VR_IY][at] = iy; A.plane[GFW_VR_IZ][at] = iz;
    A.plane[GFW_VR_IXX][at] = ixx; A.plane[GFW_VR_IXY][at] = ixy; A.plane[GFW_VR_IYY][at] = iyy;
    A.plane[GFW_VR_IXZ][at] = ixz; A.plane[GFW_VR_IYZ][at] = iyz;
    A.plane[GFW_VR_DU][at] = 0.0f; A.plane[GFW_VR_DV][at] = 0.0f;
}

// The smoothness weight s of a pixel inside the level: forward differences of (u + du, v + dv), zero across the last column / row
struct GfwVarrefField { const float *U, *du, *dv; int w, h; float alpha; };
__device__ __forceinline__ void gfw_varref_pq(const GfwVarrefField &F, int x, int y, float &p, float &q) {
    const size_t at = (size_t)y * (size_t)F.w + (size_t)x;
    p = F.U[at * 2] + F.du[at]; q = F.U[at * 2 + 1] + F.dv[at];
}
__device__ __forceinline__ float gfw_varref_s(const GfwVarrefField &F, int x, int y) {
    float p, q, pr, qr, pd, qd, fxp = 0.0f, fxq = 0.0f, fyp = 0.0f, fyq = 0.0f;
    gfw_varref_pq(F, x, y, p, q);
    if (x + 1 < F.w) { gfw_varref_pq(F, x + 1, y, pr, qr); fxp = pr - p; fxq = qr - q; }
    if (y + 1 < F.h) { gfw_varref_pq(F, x, y + 1, pd, qd); fyp = pd - p; fyq = qd - q; }
    return F.alpha / sqrtf(((((fxp * fxp) + (fyp * fyp)) + (fxq * fxq)) + (fyq * fyq)) + GFW_VARREF_EPS2);
}

// Once per fixed-point iteration: both data weights, the system's coefficients with the smoothness weights on the diagonal, the right-hand side with the field's
// Laplacian, and the pixel's right and down link weights
__global__ __launch_bounds__(256) void gfw_varref_coeff_kernel(const GfwVarrefArgs A) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x), pair = (int)blockIdx.y;
    const int w = A.w, h = A.h;
    if (idx >= w * h) return;
    const int x = idx % w, y = idx / w;
    const size_t first = (size_t)pair * (size_t)w * (size_t)h, at = first + (size_t)idx;
    const float Ix = A.plane[GFW_VR_IX][at], Iy = A.plane[GFW_VR_IY][at], Iz = A.plane[GFW_VR_IZ][at], Ixx = A.plane[GFW_VR_IXX][at], Ixy = A.plane[GFW_VR_IXY][at];
    const float Iyy = A.plane[GFW_VR_IYY][at], Ixz = A.plane[GFW_VR_IXZ][at], Iyz = A.plane[GFW_VR_IYZ][at], du = A.plane[GFW_VR_DU][at], dv = A.plane[GFW_VR_DV][at];
    // brightness constancy
    const float n = ((Ix * Ix) + (Iy * Iy)) + GFW_VARREF_ZETA;
    const float k = (Iz + (Ix * du)) + (Iy * dv);
    const float wt = (A.delta / sqrtf(((k * k) / n) + GFW_VARREF_EPS2)) / n;
    float a11 = (wt * Ix) * Ix, a12 = (wt * Ix) * Iy, a22 = (wt * Iy) * Iy, b1 = -((wt * Iz) * Ix), b2 = -((wt * Iz) * Iy);
    // gradient constancy
    const float nx = ((Ixx * Ixx) + (Ixy * Ixy)) + GFW_VARREF_ZETA, ny = ((Iyy * Iyy) + (Ixy * Ixy)) + GFW_VARREF_ZETA;
    const float kx = (Ixz + (Ixx * du)) + (Ixy * dv), ky = (Iyz + (Ixy * du)) + (Iyy * dv);
    const float wg = A.gamma / sqrtf((((kx * kx) / nx) + ((ky * ky) / ny)) + GFW_VARREF_EPS2);
    a11 = a11 + (wg * (((Ixx * Ixx) / nx) + ((Ixy * Ixy) / ny)));
    a12 = a12 + (wg * (((Ixx * Ixy) / nx) + ((Ixy * Iyy) / ny)));
    a22 = a22 + (wg * (((Ixy * Ixy) / nx) + ((Iyy * Iyy) / ny)));
    b1 = b1 - (wg * (((Ixx * Ixz) / nx) + ((Ixy * Iyz) / ny)));
    b2 = b2 - (wg * (((Ixy * Ixz) / nx) + ((Iyy * Iyz) / ny)));
    // smoothness: the link weights are means of the two pixels' s; no link leaves the level
    GfwVarrefField F;
    F.U = A.U + first * 2; F.du = A.plane[GFW_VR_DU] + first; F.dv = A.plane[GFW_VR_DV] + first; F.w = w; F.h = h; F.alpha = A.alpha;
    const float s = gfw_varref_s(F, x, y);
    const float wr = x + 1 < w ? (s + gfw_varref_s(F, x + 1, y)) * 0.5f : 0.0f, wl = x > 0 ? (gfw_varref_s(F, x - 1, y) + s) * 0.5f : 0.0f;
    const float wd = y + 1 < h ? (s + gfw_varref_s(F, x, y + 1)) * 0.5f : 0.0f, wu = y > 0 ? (gfw_varref_s(F, x, y - 1) + s) * 0.5f : 0.0f;
    const float ws = ((wr + wl) + wd) + wu;
    const float *ur = F.U + ((size_t)y * w + gfw_image_clamp(x + 1, w)) * 2, *ul = F.U + ((size_t)y * w + gfw_image_clamp(x - 1, w)) * 2;
    const float *ud = F.U + ((size_t)gfw_image_clamp(y + 1, h) * w + x) * 2, *uu = F.U + ((size_t)gfw_image_clamp(y - 1, h) * w + x) * 2;
    const float u = F.U[(size_t)idx * 2], v = F.U[(size_t)idx * 2 + 1];
    A.plane[GFW_VR_A11][at] = a11 + ws; A.plane[GFW_VR_A12][at] = a12; A.plane[GFW_VR_A22][at] = a22 + ws;
    A.plane[GFW_VR_B1][at] = b1 + ((((wr * (ur[0] - u)) + (wl * (ul[0] - u))) + (wd * (ud[0] - u))) + (wu * (uu[0] - u)));
    A.plane[GFW_VR_B2][at] = b2 + ((((wr * (ur[1] - v)) + (wl * (ul[1] - v))) + (wd * (ud[1] - v))) + (wu * (uu[1] - v)));
    A.plane[GFW_VR_WR][at] = wr; A.plane[GFW_VR_WD][at] = wd;
}

// One colour of one SOR iteration: lane i of row y owns x = 2 i + ((y + colour) & 1)
__global__ __launch_bounds__(256) void gfw_varref_sor_kernel(const GfwVarrefArgs A, int colour) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x), pair = (int)blockIdx.y;
    const int w = A.w, h = A.h, hw = (w + 1) >> 1;
    if (idx >= hw * h) return;
    const int y = idx / hw, x = 2 * (idx % hw) + ((y + colour) & 1);
    if (x >= w) return;
    const size_t first = (size_t)pair * (size_t)w * (size_t)h, at = first + (size_t)y * w + x;
    const size_t r = first + (size_t)y * w + gfw_image_clamp(x + 1, w), l = first + (size_t)y * w + gfw_image_clamp(x - 1, w);
    const size_t d = first + (size_t)gfw_image_clamp(y + 1, h) * w + x, t = first + (size_t)gfw_image_clamp(y - 1, h) * w + x;
    float *DU = A.plane[GFW_VR_DU], *DV = A.plane[GFW_VR_DV];
    const float wr = A.plane[GFW_VR_WR][at], wl = x > 0 ? A.plane[GFW_VR_WR][l] : 0.0f, wd = A.plane[GFW_VR_WD][at], wu = y > 0 ? A.plane[GFW_VR_WD][t] : 0.0f;
    const float su = (((wr * DU[r]) + (wl * DU[l])) + (wd * DU[d])) + (wu * DU[t]);
    const float sv = (((wr * DV[r]) + (wl * DV[l])) + (wd * DV[d])) + (wu * DV[t]);
    const float du = DU[at], dv = DV[at], a12 = A.plane[GFW_VR_A12][at];
    const float du2 = du + (A.omega * ((((su + A.plane[GFW_VR_B1][at]) - (a12 * dv)) / A.plane[GFW_VR_A11][at]) - du));
    const float dv2 = dv + (A.omega * ((((sv + A.plane[GFW_VR_B2][at]) - (a12 * du2)) / A.plane[GFW_VR_A22][at]) - dv));
    DU[at] = du2; DV[at] = dv2;
}

// U = (u + du, v + dv) in place
__global__ __launch_bounds__(256) void gfw_varref_apply_kernel(const GfwVarrefArgs A) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x), pair = (int)blockIdx.y;
    if (idx >= A.w * A.h) return;
    const size_t at = (size_t)pair * (size_t)A.w * (size_t)A.h + (size_t)idx;
    float *o = A.U + at * 2;
    o[0] = o[0] + A.plane[GFW_VR_DU][at]; o[1] = o[1] + A.plane[GFW_VR_DV][at];
}

static inline dim3 gfw_varref_grid(size_t lanes, int n_pairs) { return dim3((unsigned)((lanes + 255) / 256), (unsigned)n_pairs); }
hipError_t gfw_launch_varref_prepare(const GfwVarrefArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_varref_prepare_kernel, gfw_varref_grid((size_t)A.w * A.h, A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_varref_coeff(const GfwVarrefArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_varref_coeff_kernel, gfw_varref_grid((size_t)A.w * A.h, A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
hipError_t gfw_launch_varref_sor(const GfwVarrefArgs &A, int colour, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_varref_sor_kernel, gfw_varref_grid((size_t)((A.w + 1) >> 1) * A.h, A.n_pairs), dim3(64, 4), 0, s, A, colour);
    return hipGetLastError();
}
hipError_t gfw_launch_varref_apply(const GfwVarrefArgs &A, hipStream_t s) {
    if (A.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(gfw_varref_apply_kernel, gfw_varref_grid((size_t)A.w * A.h, A.n_pairs), dim3(64, 4), 0, s, A);
    return hipGetLastError();
}
