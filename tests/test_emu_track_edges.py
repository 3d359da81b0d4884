"""The per-row matrix builder's kernels (gfw_matrices.hip with gfw_quat.h and gfw_spline.h) host-interpreted (tests/_emu.py) over the case table of
tests/_trackcase.py — the edges of quat_at, offset_at, slerp, f2i64 and catmull_rom_at: track ends, hemisphere flips, coarse / stationary / short / unnormalised
tracks, exact hits and half-microseconds, sync offsets outside their table, non-finite timestamps, video rotation, row counts around the 64-lane workgroup, splines
shorter than the sensor — against the float64 statement (tests/_hoststmt.py, itself held to a 50-digit one in tests/test_track_statement.py).  The CPU-tier twin
of tests/test_gpu_track_edges.py: same inputs, same bars (<= 2 ULP of f32 on the matrix entries, <= 1 ULP on the stabiliser terms, cos / sin slots the host
libm's of the row's f32 angle, slots 9..15 exactly 0 / 1 / 0 without terms).  A failure here is a logic bug in the three files named first."""
import numpy as np
import pytest

from gyroflow_amd import synthetic as S
import _emu
import _oracle as O
import _trackcase as TC
from test_gpu_matrix_builder import ulps


def build(c, **kw):
    a = dict(timestamps_ms=c.ts, frame_readout_time_ms=c.readout, rows=c.rows, readout_dim=c.dim, video_rotation_deg=c.rot, framebuffer_inverted=c.inverted,
             offsets=c.offsets, duration_ms=c.duration, stab=c.stab)
    a.update(kw)
    return _emu.build_matrices(c.org, c.sm, TC.NK, **a)


@pytest.mark.parametrize("name", TC.NAMES)
def test_rows_match_the_f64_statement(name):
    c = TC.CASES[name]
    ref = TC.reference(name)
    got = build(c)[0]
    TC.check_rows(name, got, ref, c.stab, TC.oracle_libm())
    if name in ("ends_before", "ends_after") or name.startswith("nonfinite_"):
        assert np.all(got.view(np.uint32) == got[0].view(np.uint32))                          # every row is the one clamped lookup


@pytest.mark.parametrize("flip", sorted(TC.TWINS))
def test_q_and_minus_q_are_one_rotation(flip):
    a, b = build(TC.CASES[flip])[0], build(TC.CASES[TC.TWINS[flip]])[0]
    scale = np.abs(b[:, :9]).max(axis=1, keepdims=True) * 1e-4
    assert ulps(a[:, :9], b[:, :9], scale).max() <= 2.0


def test_a_batch_of_frames_with_1_65_and_48_rows():
    c = TC.CASES[TC.BATCH_TRACKS]
    batch = build(c, timestamps_ms=[f[0] for f in TC.BATCH], rows=[f[1] for f in TC.BATCH], readout_dim=[f[2] for f in TC.BATCH])
    assert batch.shape == (3, 65, 16)
    for k, (ts, rows, dim) in enumerate(TC.BATCH):
        single = build(c, timestamps_ms=ts, rows=rows, readout_dim=dim)[0]
        assert np.array_equal(batch[k, :rows].view(np.uint32), single.view(np.uint32)), k
        assert np.all(batch[k, rows:].view(np.uint32) == 0), k                                 # a lane past its frame's rows writes nothing
        TC.check_rows("batch frame %d" % k, single, TC.batch_reference(k), None, TC.oracle_libm())


def test_warp_with_the_coarse_flipped_rows_is_bit_exact_against_the_oracle_fed_the_same_rows():
    fr = S.SyntheticFrame("YUV422P16LE", TC.W, TC.H, seed=9)
    rows = build(TC.CASES[TC.WARP_CASE])[0]
    fr.matrices = np.ascontiguousarray(rows[:, :14])
    for a, b in zip(O.run_frame(fr), _emu.run_frame(fr)):
        assert np.array_equal(a, b)
