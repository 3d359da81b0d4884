// gfw_matrices_host.h — host only: the device form of gfw_frame_stab, one frame's and a clip's table, as gfw_build_matrices_stab, gfw_build_matrices_batch_stab and
// gfw_zoom_fovs_stab stage it.  Included behind gfw_matrices.h (GfwStab) by gfw_api.hip and by whatever else stages a call for those kernels; no kernel's
// translation unit sees it, it calls nothing of HIP and reports no errors (the entry points validate).
#pragma once
#include <string.h>
#include "gfw_layout.h"

inline size_t stab_point_bytes(const gfw_frame_stab *stab) { return ((size_t)stab->ibis_count + (size_t)stab->ois_count) * 32; }
// The device form of a frame's stabiliser data; its control points are copied to `h_points` (pinned), which the caller uploads to `d_points`.  y_sign: the
// framebuffer sign of the matrix path (frame_transform.rs:234-241), 1.0 for at_timestamp_for_points (:413-416)
inline GfwStab stab_device(const gfw_frame_stab *stab, double y_sign, void *h_points, const void *d_points) {
    const size_t nb0 = (size_t)stab->ibis_count * 32, nb1 = (size_t)stab->ois_count * 32;
    if (nb0) memcpy(h_points, stab->ibis, nb0);
    if (nb1) memcpy((char *)h_points + nb0, stab->ois, nb1);
    GfwStab S;
    S.offset = stab->offset; S.sensor_h = stab->sensor_size[1]; S.crop_y = stab->crop_area[1]; S.crop_h = stab->crop_area[3];
    S.scale_x = stab->width / stab->crop_area[2] / stab->pixel_pitch[0];
    S.scale_y = stab->height / stab->crop_area[3] / stab->pixel_pitch[1] * y_sign;
    S.height = stab->height;
    S.ibis = (const double *)d_points; S.ois = (const double *)((const char *)d_points + nb0); S.ibis_n = stab->ibis_count; S.ois_n = stab->ois_count;
    return S;
}
inline const GfwStab kNoStab = {0, 0, 0, 0, 0, 0, 0, nullptr, nullptr, -1, -1};

// A clip's table: [count] GfwStab, then the control points of the frames that have an entry, back to back (IBIS then OIS of each).
struct GfwStabTable { size_t o_table, o_points; };
inline size_t gfw_stab_points_total(const gfw_frame_stab *const *stabs, int count) {
    size_t bytes = 0;
    for (int i = 0; i < count; ++i) if (stabs[i]) bytes += stab_point_bytes(stabs[i]);
    return bytes;
}
inline GfwStabTable gfw_stab_table_layout(BlockLayout &L, int count, size_t point_bytes) {
    GfwStabTable S;
    S.o_table = L.add(sizeof(GfwStab) * (size_t)count); S.o_points = L.add(point_bytes);
    return S;
}
// Fills the table in the block at (h, d).  `timings`: the frames' descriptors, whose framebuffer_inverted gives the matrix path's sign — nullptr: 1.0.  -> the kernels' argument
inline const GfwStab *gfw_stab_table_fill(const GfwStabTable &S, const gfw_frame_stab *const *stabs, const gfw_frame_timing *timings, int count, char *h, const char *d) {
    GfwStab *hs = (GfwStab *)(h + S.o_table);
    size_t at = S.o_points;
    for (int i = 0; i < count; ++i) {
        if (!stabs[i]) { hs[i] = kNoStab; continue; }
        hs[i] = stab_device(stabs[i], timings && timings[i].framebuffer_inverted ? -1.0 : 1.0, h + at, d + at);
        at += stab_point_bytes(stabs[i]);
    }
    return (const GfwStab *)(d + S.o_table);
}
