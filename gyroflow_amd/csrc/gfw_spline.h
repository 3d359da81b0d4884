// gfw_spline.h — the Catmull-Rom evaluation of the stabiliser splines (file_metadata.camera_stab_data: IBIS / OIS positions along the sensor readout), shared by
// the per-row matrix builder (gfw_matrices.hip: frame_transform.rs:270-289) and the zoom search's per-point shifts (gfw_zoom.hip: frame_transform.rs:412-435).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// CatmullRom<Vector3<f64>>::interpolate (gyro_source/splines.rs:22-84) over `n` control points (position, x, y, z);
// false = None (the caller substitutes the default, zero)
__device__ bool catmull_rom_at(const double *pts, int n, double t, double out[3]) {
    if (n < 2 || !(t == t)) return false;
    // search_lower_cp: binary_search_by(partial_cmp): Ok(i) exact hit, Err(i) insertion point
    int lo = 0, hi = n;                                           // first index with position >= t
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (pts[mid * 4] < t) lo = mid + 1; else hi = mid; }
    int lower;
    if (lo < n && pts[lo * 4] == t) { if (lo == n - 1) return false; lower = lo; }
    else { if (lo >= n || lo == 0) return false; lower = lo - 1; }
    if (lower + 1 >= n) return false;
    const double *pa = pts + (size_t)lower * 4, *pb = pa + 4;
    const double k = (t - pa[0]) / (pb[0] - pa[0]);               // normalize
    for (int c = 0; c < 3; ++c) {
        const double a = pa[1 + c], b = pb[1 + c];
        const double x = (lower <= 0) ? a * 2.0 - b : pa[1 + c - 4];
        const double y = (lower + 2 >= n) ? b * 2.0 - a : pb[1 + c + 4];
        out[c] = ((((a * 3.0 - x) - b * 3.0) + y) * 0.5) * k * k * k + ((b - x) * 0.5) * k + a + (((b * 4.0 + a * -5.0 + x + x) - y) * 0.5) * k * k;
    }
    return true;
}

}  // namespace
