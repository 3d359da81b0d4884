// emu_matrices_stab_driver.inc — TEST INFRASTRUCTURE: gfw_build_matrices_stab_kernel (gfw_matrices.hip, compiled for the host above), the row kernel of
// gfw_build_matrices_batch_stab that reads each frame's stabiliser data from a table, beside what emu_matrices_driver.inc drives: a loop over the launch grid of
// gfw_launch_build_matrices_stab stands in for the device.  The table is the entry point's own (gfw_matrices_host.h).
#include "emu_matrices_driver.inc"
#include "../../gyroflow_amd/csrc/gfw_matrices_host.h"

// stabs: [frames] gfw_frame_stab pointers as gfw_build_matrices_batch_stab takes them (NULL: the frame has no stabiliser data)
extern "C" int gfw_emu_build_matrices_stab(const int64_t *org_ts, const double *org_q, int org_n, const int64_t *sm_ts, const double *sm_q, int sm_n,
                                           const int64_t *off_ts, const double *off_ms, int off_n, double duration_ms,
                                           const gfw_frame_timing *Fs, int frames, int max_rows, float *out, size_t table_floats, const gfw_frame_stab *const *stabs) {
    GfwTracks T{org_ts, org_q, org_n, sm_ts, sm_q, sm_n, off_ts, off_ms, off_n, duration_ms};
    BlockLayout L;
    const GfwStabTable S = gfw_stab_table_layout(L, frames, gfw_stab_points_total(stabs, frames));
    std::vector<uint64_t> block(L.total / 8);                                 // ONE block of exactly the layout's bytes ("device" = host memory)
    const GfwStab *table = gfw_stab_table_fill(S, stabs, Fs, frames, (char *)block.data(), (const char *)block.data());
    std::vector<double> prefix((size_t)frames * 4);
    static EmuLane lane;
    emu_cur = &lane;
    lane.bdim = dim3(64, 1, 1);
    lane.gdim = dim3((frames + 63) / 64, 1, 1);
    for (unsigned b = 0; b < lane.gdim.x; ++b) for (unsigned t = 0; t < 64; ++t) {
        lane.bid = dim3(b, 0, 0); lane.tid = dim3(t, 0, 0);
        gfw_build_prefix_kernel(T, Fs, frames, prefix.data());
    }
    lane.gdim = dim3((max_rows + 63) / 64, frames, 1);
    for (unsigned f = 0; f < (unsigned)frames; ++f) for (unsigned b = 0; b < lane.gdim.x; ++b) for (unsigned t = 0; t < 64; ++t) {
        lane.bid = dim3(b, f, 0); lane.tid = dim3(t, 0, 0);
        gfw_build_matrices_stab_kernel(T, Fs, prefix.data(), out, table_floats, table);
    }
    return 0;
}
