"""The row kernel of gfw_build_matrices_batch_stab (gfw_matrices.hip: gfw_build_matrices_stab_kernel — each frame's stabiliser data read from a device table),
host-interpreted (tests/_zoomstab.py, tests/emu/emu_matrices_stab_driver.inc): every frame's table equals, bit for bit, what the single-frame kernel
(gfw_build_matrices_kernel, the frame's GfwStab by value: tests/_emu.build_matrices) writes for that frame — m[9..13], the cos / sin slots, the
framebuffer_inverted sign and sensor flip, suppress_rotation 0 / 1 / 2, frames without an entry — and holds the bar of tests/test_emu_matrices.py against the f64
host statement (<= 2 ULP of f32 on the matrix entries, <= 1 ULP on the stabiliser terms)."""
import numpy as np

from gyroflow_amd import synthetic as S
import _emu
import _hoststmt as HS
import _zoomstab as ZS
from test_gpu_matrix_builder import ulps

W, H = 320, 192


def test_every_table_of_a_batch_equals_the_single_frame_kernel_bit_for_bit():
    fr = S.SyntheticFrame("YUV422P16LE", W, H, seed=3, pixels=False)
    org, sm = S.sampled_track(11, 0.0, 2000.0, 1000.0), S.sampled_track(12, 0.0, 2000.0, 200.0, scale=0.25)
    nk = S.new_k(fr.lens, 1.0, W, H)
    offsets = (np.array([0, 700000, 1500000], dtype=np.int64), np.array([3.5, -2.25, 6.0]))
    n = 14
    timings, stabs = ZS.batch_case(n, W, H, nk)
    batch = ZS.emu_build_matrices_stab(org, sm, timings, stabs, H, offsets=offsets, duration_ms=2000.0)
    seen = set()
    for k in range(n):
        t = timings[k]
        single = _emu.build_matrices(org, sm, nk, t.timestamp_ms, t.frame_readout_time_ms, H, H, framebuffer_inverted=bool(t.framebuffer_inverted),
                                     per_frame_offset_ms=t.per_frame_time_offset_ms, offsets=offsets, duration_ms=2000.0, suppress_rotation=t.suppress_rotation, stab=stabs[k])[0]
        assert np.array_equal(batch[k].view(np.uint32), single.view(np.uint32)), k
        host = HS.row_matrices_from_tracks(org, sm, nk, t.timestamp_ms, t.frame_readout_time_ms, H, H, framebuffer_inverted=bool(t.framebuffer_inverted),
                                           per_frame_offset_ms=t.per_frame_time_offset_ms, offsets=offsets, duration_ms=2000.0, suppress_rotation=t.suppress_rotation, stab=stabs[k])
        scale = np.abs(host[:, :9]).max(axis=1, keepdims=True) * 1e-4
        assert ulps(batch[k][:, :9], host[:, :9], scale).max() <= 2.0, k
        assert ulps(batch[k][:, 9:14], host[:, 9:14], np.full((H, 1), 1e-6)).max() <= 1.0, k
        has_terms = stabs[k] is not None and t.suppress_rotation != 2
        assert (np.abs(batch[k][:, 9:14]).max() > 0.05) == has_terms, k                      # (0 without: exactly)
        if not has_terms:
            assert np.all(batch[k][:, 14] == 1.0) and np.all(batch[k][:, 15] == 0.0), k
        seen.add((stabs[k] is not None, t.framebuffer_inverted, t.suppress_rotation))
    assert {(True, 0, 0), (True, 1, 0), (False, 0, 0), (False, 1, 0)} <= seen and {s[2] for s in seen} == {0, 1, 2}, seen
    assert not np.array_equal(batch[0], batch[3])
