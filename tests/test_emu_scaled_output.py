"""Renders at another output size than the source's, through the fused kernel's own source interpreted on the host (tests/_emu.py): the CPU twin of
tests/test_gpu_scaled_output.py over the same shape table (tests/_shapes.py).

The output size drives the fused kernel separately from the input size: the chroma ratio and the tile counts come from the output planes, the source map
constants from the input planes, the first pass's rho range from the output frame's corners while its row is clamped to the SOURCE rows, and the lattice of the
first pass reaches a tile beyond the last OUTPUT pixel.  Every frame here is compared bit for bit with the oracle fed the same parameters, and the audit
instantiation re-derives the exact row of every pixel it certified."""
import numpy as np
import pytest

from gyroflow_amd import abi
import _emu
import _oracle as O
from _shapes import CONTROL, MODELS, SHAPES, fused_expected, scaled_frame, sizes


def assert_frames_equal(ref, got, what):
    for i, (a, b) in enumerate(zip(ref, got)):
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError("%s plane %d: %d bytes differ (first at %d: ref %d got %d)" % (what, i, bad.size, bad[0], a[bad[0]], b[bad[0]]))


@pytest.mark.parametrize("baked", [True, False])
@pytest.mark.parametrize("fmt", ["YUV422P16LE", "NV12"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_frame_at_another_output_size_equals_the_oracle(name, fmt, baked):
    fr = scaled_frame(fmt, name, seed=0x5CA1 + len(name), background_rgba=(0.2, 0.6, 0.4, 1.0))
    assert _emu.fused_eligible(fr) == fused_expected(name, fmt), name
    if not fused_expected(name, fmt):
        # (the other side of the boundary: an even output of the same source takes the fused kernel — the first case of this file's table does)
        assert fr.planes[1]["out_size"][0] * 2 != fr.out_size[0]
        return
    assert_frames_equal(O.run_frame(fr), _emu.run_frame(fr, baked=baked), "%s %s baked=%s" % (name, fmt, baked))


@pytest.mark.parametrize("name", ["down_half", "portrait"])
def test_five_frame_clip_launch_at_another_output_size(name):
    frames = [scaled_frame("YUV422P16LE", name, seed=0xC11 + j, timestamp_ms=1000.0 + 33.3 * j) for j in range(5)]
    outs = _emu.run_frames(frames)
    for j, fr in enumerate(frames):
        assert_frames_equal(O.run_frame(fr), outs[j], "%s clip launch frame %d" % (name, j))


def _audit_format(name):
    return "YUV444P16LE" if name == "odd_out" else "YUV422P16LE"          # (an odd output is fused only without subsampled chroma)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", sorted(SHAPES) + sorted(CONTROL))
def test_every_certificate_at_another_output_size(name, model):
    """The audit instantiation over every shape and each model the certified first pass serves (fisheye: table over rho, restated in _emu.p1_table; GoPro, Sony,
    the generic polynomial: table over r from the library's host code).  Not one wrong certificate, every output pixel certified or queued, the measured gap inside E."""
    fr = scaled_frame(_audit_format(name), name, fov_s=1.0, model=model, seed=0xA0D1, readout_ms=14.0)
    p0 = fr.planes[0]["params"]
    assert p0.matrix_count == fr.height and (p0.output_width, p0.output_height) == sizes(name)[1]
    p1 = _emu.p1_table(p0, fr.matrices, p0.matrix_count) if model == "opencv_fisheye" else _emu.p1_table_radial(fr)
    assert p1 is not None, "the host must certify %s at %s" % (model, name)
    outs, a = _emu.run_frames([fr], audit=True)
    ow, oh = sizes(name)[1]
    print("%-20s %-20s certified %.4f  gap / E %.3f" % (name, model, a["certified"] / float(ow * oh), a["gap_px"] / a["eps_px"]))
    assert a["wrong"] == 0 and a["queue_overflow"] == 0 and a["out_of_range"] == 0, a
    assert a["certified"] + a["queued"] + a["queue_overflow"] == ow * oh, a
    assert a["certified"] > 0 and a["gap_px"] < a["eps_px"], a
    assert_frames_equal(O.run_frame(fr), outs[0], "%s %s audit build" % (name, model))


@pytest.mark.parametrize("name", ["down_half", "portrait"])
def test_every_certificate_of_a_horizontal_shutter_at_another_output_size(name):
    """A horizontal shutter: one matrix per SOURCE column, the output's columns mapped onto them."""
    fr = scaled_frame("NV12", name, seed=0xA0D2, readout_ms=-12.0, horizontal_rs=True)
    p0 = fr.planes[0]["params"]
    assert p0.matrix_count == fr.width and p0.flags & abi.FLAG_HORIZONTAL_RS
    assert _emu.p1_table(p0, fr.matrices, p0.matrix_count) is not None
    outs, a = _emu.run_frames([fr], audit=True)
    ow, oh = SHAPES[name][1]
    assert a["wrong"] == 0 and a["queue_overflow"] == 0 and a["out_of_range"] == 0, a
    assert a["certified"] + a["queued"] == ow * oh and a["certified"] > 0 and a["gap_px"] < a["eps_px"], a
    assert_frames_equal(O.run_frame(fr), outs[0], "%s horizontal shutter audit build" % name)
