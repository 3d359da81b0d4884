"""The pair's second matrix row (gfw_frame.hip, GFW_PAIR_ROW): the branch-free lane-row of a pixel PAIR fetches the second pixel's row only in the lanes whose two rows
differ and copies the first pixel's in the others.  Equal rows are the same memory, so every output byte must stay what it was: each clip below runs through the
host-interpreted kernel source with the switch on and off, the two outputs must be equal, and both must be the oracle's.

Each clip stands for a regime of "the two rows differ", and says which: the share of differing pairs is computed from the oracle's own first pass
(tests/_pair_rows.py) and asserted — none (one matrix; a flat first pass: the wave-uniform skip), a third (lanes on both sides of the branch in nearly every wave),
nearly all (horizontal rolling shutter), and rows that differ before the clamp to the table and are equal after it.  160 x 96 (one full wave and one with dead lanes
per line) or 200 x 96, launches of four frames."""
import contextlib

import numpy as np
import pytest

from gyroflow_amd import synthetic as S
import _emu as E
import _emu_perframe as EP
import _emu_perlens as EL
import _oracle as O
import _pair_rows as P

W, H, N = 160, 96, 4
SWITCH = (0, 1)


@contextlib.contextmanager
def pair_row(value):
    """the interpreter's builds with GFW_PAIR_ROW=value (one more definition in front of the kernel source, as GFW_JIT_DEFS adds it to the library's own builds)"""
    build, paths = E.build, []

    def with_switch(defs, header, **kw):
        paths.append(build(dict(defs, GFW_PAIR_ROW=value), header, **kw))
        return paths[-1]
    E.build = with_switch
    try:
        yield paths
    finally:
        E.build = build


def clip(case, fmt, w=W, h=H, **kw):
    return [P.case_frame(case, fmt, w, h, f, **kw) for f in range(N)]


def on_off_and_oracle(frames, run=E.run_frames, what=""):
    got = {}
    for v in SWITCH:
        with pair_row(v):
            got[v] = run(frames)
    for f, fr in enumerate(frames):
        ref = O.run_frame(fr)
        for p in range(len(ref)):
            for v in SWITCH:
                a, b = ref[p], got[v][f][p]
                assert np.array_equal(a, b), "%s GFW_PAIR_ROW=%d frame %d plane %d: %d bytes differ from the oracle" % (what, v, f, p, int(np.count_nonzero(a != b)))
            assert np.array_equal(got[SWITCH[0]][f][p], got[SWITCH[-1]][f][p])
    return got


def test_the_switch_reaches_the_interpreted_source():
    """a build per value: the definition is part of the build's key, and the source asks for it"""
    fr = P.case_frame("roll", "YUV422P16LE", W, H)
    built = []
    for v in SWITCH:
        with pair_row(v) as paths:
            E.run_frames([fr])
        built.append(tuple(paths))
    assert all(len(b) == 1 for b in built) and len(set(built)) == len(SWITCH), built
    assert "#if GFW_PAIR_ROW" in E.kernel_source() or "GFW_PAIR_ROW != 0" in E.kernel_source()


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12"])
def test_one_matrix_the_comparison_folds(fmt):
    """(a) no rolling shutter: every pixel's row is row 0"""
    frames = clip("single", fmt)
    assert all(fr.matrices.shape[0] == 1 for fr in frames)
    on_off_and_oracle(frames, what=fmt)


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12"])
def test_no_pair_differs_the_wave_skips_the_fetch(fmt):
    """(b) rolling shutter over a flat first pass: 192 rows in use, and not one pair of the clip straddles two of them"""
    frames = clip("flat", fmt)
    assert frames[0].matrices.shape[0] == 2 * H and not np.array_equal(frames[0].matrices[0], frames[0].matrices[-1])
    rows = P.pixel_rows(frames[0])
    assert rows.min() == H // 2 and rows.max() == H // 2 + H - 1
    for pairs, quads, waves in P.clip_shares(frames):
        assert pairs == 0.0 and waves == 0.0
    on_off_and_oracle(frames, what=fmt)


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12"])
def test_a_rolled_frame_lanes_on_both_sides(fmt):
    """(c) 25 degrees of roll, 30 ms readout: about sin 25 deg of the pairs differ, and so does some pair of nine waves in ten"""
    frames = clip("roll", fmt)
    for pairs, quads, waves in P.clip_shares(frames):
        assert 0.05 < pairs < 0.95 and waves > 0.9, (pairs, quads, waves)
    on_off_and_oracle(frames, what=fmt)


def test_horizontal_rolling_shutter_nearly_every_pair_differs():
    """(d) the row index follows x"""
    frames = clip("hrs", "YUV422P16LE")
    assert frames[0].matrices.shape[0] == W
    for pairs, quads, waves in P.clip_shares(frames):
        assert pairs > 0.9 and waves == 1.0, (pairs, quads, waves)
    on_off_and_oracle(frames)


def test_rows_that_differ_before_the_clamp_and_not_after():
    """(e) the first pass's row is tilted past the table's last row: over the lower part of the frame distinct rounded rows clamp to matrix_count - 1, and the
    comparison must see the clamped ones (the fetch addresses are made of them)"""
    frames = clip("clamp", "YUV422P16LE")
    for fr in frames:
        raw, rows = P.pixel_rows(fr, clamped=False), P.pixel_rows(fr)
        assert raw.max() > H + 10 and rows.max() == H - 1
        d_raw, d = raw[:, 0::2] != raw[:, 1::2], rows[:, 0::2] != rows[:, 1::2]
        assert np.count_nonzero(d_raw & ~d) > 100 and np.count_nonzero(d) > 100, (np.count_nonzero(d_raw & ~d), np.count_nonzero(d))
    on_off_and_oracle(frames)


def test_a_width_that_is_no_multiple_of_the_tile():
    """(f) 200 columns: the second wave of a line has 28 dead lanes"""
    frames = clip("roll", "YUV422P16LE", w=200)
    for pairs, quads, waves in P.clip_shares(frames):
        assert 0.05 < pairs < 0.95
    on_off_and_oracle(frames)


@pytest.mark.parametrize("interp", [4, 8])
def test_bicubic_and_lanczos4_on_the_rolled_frame(interp):
    """(g) the LUT samplers share the row's head with the bilinear one but keep their six unconditional fetches (the switch is compiled for bilinear only): either
    value of it must leave their clips the oracle's"""
    on_off_and_oracle(clip("roll", "YUV422P16LE", interp=interp), what="interpolation %d" % interp)


def test_the_per_frame_flavour_on_the_rolled_frame():
    """(h) gfw_undistort_clip_params' kernel: the field of view moves from frame to frame"""
    frames = [P.case_frame("roll", "YUV422P16LE", W, H, f, fov=1.0 + 0.04 * f) for f in range(N)]
    for pairs, quads, waves in P.clip_shares(frames):
        assert 0.05 < pairs < 0.95
    on_off_and_oracle(frames, run=EP.run_frames_pf)


def test_the_moving_lens_flavour_on_the_rolled_frame():
    """(h) gfw_undistort_clip_lens' kernel: focal length, centre and coefficients move from frame to frame (its first pass is the exact one)"""
    def lens(f):
        l = S.gopro_style_lens(W, H)
        l["f"] = ((0.47 + 0.03 * f) * W, (0.47 + 0.03 * f) * W * 1.002)
        l["c"] = (W / 2.0, H / 2.0)
        l["k"] = [0.045 + 0.01 * f, 0.02 - 0.004 * f, -0.02, 0.006] + [0.0] * 8
        return l
    frames = [P.case_frame("roll", "YUV422P16LE", W, H, f, fov=1.0 + 0.03 * f, lens=lens(f)) for f in range(N)]
    for pairs, quads, waves in P.clip_shares(frames):
        assert 0.05 < pairs < 0.95
    on_off_and_oracle(frames, run=EL.run_frames_pl)
