"""Renders at another output size than the source's (gyroflow sets the two independently: a 4K clip exported at 1080p, a 1080p clip upscaled, 16:9 to 9:16).

One table shared by the CPU tier (tests/test_emu_scaled_output.py) and the GPU tier (tests/test_gpu_scaled_output.py).  A frame is built as the reference
builds it: ``fov = fov_s * in_w / out_w`` (stabilization.py: FrameTransform.get_fov, frame_transform.rs), the new camera centred on the OUTPUT
(``synthetic.new_k``: frame_transform.rs:37-51), and one matrix per SOURCE row (or column, horizontal shutter): ``synthetic.row_matrices`` already counts them
on the input."""
from gyroflow_amd import synthetic as S

# name -> (input w, h), (output w, h)
SHAPES = {
    "down_half": ((768, 432), (384, 216)),                 # two source rows per output row
    "up_double": ((320, 180), (640, 360)),                 # half a source row per output row
    "down_two_thirds": ((576, 324), (384, 216)),           # non-integer ratio
    "up_three_halves": ((256, 144), (384, 216)),           # non-integer ratio
    "portrait": ((384, 216), (216, 384)),                  # 16:9 -> 9:16: a tall output, far vertical rays
    "square": ((384, 216), (216, 216)),                    # aspect change; 216 is not a multiple of the 64-lane tile
    "four_three_to_wide": ((288, 216), (384, 216)),        # wider than the source
    "odd_out": ((384, 216), (383, 215)),                   # 4:2:0 / 4:2:2 chroma not an integer divisor: the per-plane kernel's
}
FULL_SIZE = {
    "down_4k_to_1080p": ((3840, 2160), (1920, 1080)),
    "up_1080p_to_4k": ((1920, 1080), (3840, 2160)),
}
CONTROL = {"same": ((384, 216), (384, 216))}                 # output = input: the control beside the audits' figures
FUSED_SHAPES = [n for n in SHAPES if n != "odd_out"]
SUBSAMPLED = {"NV12", "P010", "P010LE", "P210", "P210LE", "YUV420P", "YUV420P10LE", "YUV422P16LE"}
MODELS = ["opencv_fisheye", "gopro", "sony", "generic_polynomial"]


def sizes(name):
    return SHAPES.get(name) or FULL_SIZE.get(name) or CONTROL[name]


def fused_expected(name, fmt):
    """Subsampled chroma of an odd output has no integer divisor (383 / 192): those frames leave the fused kernel; every other shape takes it."""
    return not (name == "odd_out" and fmt in SUBSAMPLED)


def lens_for(model, w, h):
    """The lens of each model the certified first pass serves, on the SOURCE frame: the fisheye of synthetic.py, the GoPro / Sony / generic-polynomial
    coefficient sets of tests/test_gpu_pass1_radial.py (r_limit 2.5 on the radial ones)."""
    if model == "opencv_fisheye":
        return S.gopro_style_lens(w, h)
    from test_gpu_pass1_radial import closed_form_lens, gopro_lens
    return gopro_lens(w, h) if model == "gopro" else closed_form_lens(model, w, h)


def scaled_frame(fmt, name, fov_s=1.0, model="opencv_fisheye", lens=None, **kw):
    """A SyntheticFrame of shape `name`: source planes at the input size, output planes at the output size, fov scaled as get_fov scales it."""
    (iw, ih), (ow, oh) = sizes(name)
    return S.SyntheticFrame(fmt, iw, ih, fov=fov_s * iw / ow, out_size=(ow, oh), lens=lens if lens is not None else lens_for(model, iw, ih), **kw)
