"""The device-side matrix builder (gfw_build_matrices / _stab / _batch) on the MI355X over the case table of tests/_trackcase.py — the edges of quat_at, offset_at,
slerp, f2i64 and catmull_rom_at (gyroflow_amd/csrc/gfw_quat.h, gfw_spline.h) — against the float64 statement; the GPU-tier twin of
tests/test_emu_track_edges.py.  Here acos, sin, cos and round are the device library's and the f64 -> i64 conversion is the compiler's expansion, at inputs no other
test gives them: c within an ulp of 1, c < 0, NaN / infinite / 1e300 timestamps, half-microseconds of either sign.  Bars as tests/test_gpu_matrix_builder.py holds
them: <= 2 ULP of f32 on entries 0..8, <= 1 ULP on the five stabiliser terms, cos / sin slots the host libm's of the row's own f32 angle, slots 9..15 exactly
0 / 1 / 0 where a row has no terms.  One context serves every case: tracks and sync offsets are set per case."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
import _trackcase as TC
from test_gpu_matrix_builder import fetch_rows, ulps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    fr = S.SyntheticFrame("YUV422P16LE", TC.W, TC.H, seed=3)
    pl = fr.planes[0]
    b = warp.Backend(pl["params"], pl["pixel_type"], fr.model, 0, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    yield b
    b.close()


def set_case(be, c):
    be.set_quaternion_tracks(c.org, c.sm)
    if c.offsets is None:
        be.set_sync_offsets(c.duration)
    else:
        be.set_sync_offsets(c.duration, c.offsets[0], c.offsets[1])


def build(be, c):
    set_case(be, c)
    return fetch_rows(be.build_matrices(TC.NK, c.ts, c.readout, c.rows, c.dim, c.rot, c.inverted, stab=c.stab), c.rows)


@pytest.mark.parametrize("name", TC.NAMES)
def test_device_rows_match_the_f64_statement(be, name):
    c = TC.CASES[name]
    ref = TC.reference(name)
    got = build(be, c)
    TC.check_rows("%s/%s" % (c.group, name), got, ref, c.stab, TC.oracle_libm())
    if name in ("ends_before", "ends_after") or name.startswith("nonfinite_"):
        assert np.all(got.view(np.uint32) == got[0].view(np.uint32))                          # every row is the one clamped lookup


@pytest.mark.parametrize("flip", sorted(TC.TWINS))
def test_q_and_minus_q_are_one_rotation_on_the_device(be, flip):
    a, b = build(be, TC.CASES[flip]), build(be, TC.CASES[TC.TWINS[flip]])
    scale = np.abs(b[:, :9]).max(axis=1, keepdims=True) * 1e-4
    assert ulps(a[:, :9], b[:, :9], scale).max() <= 2.0


def test_a_batch_of_frames_with_1_65_and_48_rows_equals_the_single_builds(be):
    c = TC.CASES[TC.BATCH_TRACKS]
    set_case(be, c)
    n = len(TC.BATCH)
    arr = (abi.FrameTiming * n)()
    for t, (ts, rows, dim) in zip(arr, TC.BATCH):
        t.timestamp_ms, t.per_frame_time_offset_ms, t.frame_readout_time_ms = ts, 0.0, c.readout
        for i, v in enumerate(np.asarray(TC.NK, dtype=np.float64).reshape(9)):
            t.new_k[i] = v
        t.video_rotation_deg, t.rows, t.readout_dim, t.framebuffer_inverted, t.suppress_rotation = c.rot, rows, dim, 0, 0
    ptrs = (C.c_void_p * n)()
    be._check(be.lib.gfw_build_matrices_batch(be.ctx, arr, n, ptrs))
    assert ptrs[1] - ptrs[0] == 65 * 16 * 4 == ptrs[2] - ptrs[1]                            # the grid and the tables are sized by the largest frame
    batch = [fetch_rows(ptrs[k], TC.BATCH[k][1]) for k in range(n)]
    for k, (ts, rows, dim) in enumerate(TC.BATCH):
        single = fetch_rows(be.build_matrices(TC.NK, ts, c.readout, rows, dim, c.rot, c.inverted), rows)
        assert np.array_equal(batch[k].view(np.uint32), single.view(np.uint32)), k
        TC.check_rows("batch/frame %d" % k, batch[k], TC.batch_reference(k), None, TC.oracle_libm())


def test_warp_with_the_coarse_flipped_device_rows_is_bit_exact_against_the_oracle_fed_the_same_rows():
    w, h = TC.W, TC.H
    c = TC.CASES[TC.WARP_CASE]
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=9)
    outs = [pl["dst"].copy() for pl in fr.planes]
    bufs = [warp.host_buffers(pl["src"], pl["size"], o, pl["out_size"]) for pl, o in zip(fr.planes, outs)]
    params = [pl["params"] for pl in fr.planes]
    types = [pl["pixel_type"] for pl in fr.planes]
    b = warp.Backend(params[0], types[0], fr.model, 0, bufs[0])
    try:
        set_case(b, c)
        ptr = b.build_matrices(TC.NK, c.ts, c.readout, h, h)
        rows = fetch_rows(ptr, h)
        b.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        b.undistort_frame(bufs, params, types, ptr, matrix_count=h)
    finally:
        b.close()
    TC.check_rows("coarse/warp rows", rows, TC.reference(TC.WARP_CASE), None, TC.oracle_libm())
    assert not np.array_equal(rows[0, :9], rows[-1, :9])
    fr.matrices = np.ascontiguousarray(rows[:, :14])
    for a, o in zip(O.run_frame(fr), outs):
        assert np.array_equal(a, o)
