"""The destination stores of the fused kernel's branch-free row (gfw_frame.hip store_value1 / store_pair1; non-temporal since round 7, GFW_NT_STORE): the bytes must be
the oracle's wherever a frame's planes lie, and nothing may be written outside a plane's rows — the destinations are pre-filled with 0x5A, and row padding, the bytes
around every plane and the gaps between the planes of one allocation must still hold it.  Shapes: whole tiles, tiles whose last column is partial (odd chroma
widths: a wave with dead lanes), 4:2:2 / 4:2:0 / 4:4:4 planar at 8 and 16 bits, interleaved chroma, U before V, V before U, separate allocations, padded pitches,
two frames of one clip launch with different plane distances, border waves beside interior waves, and the checksum flavour, which must add what the stored bytes add.

Every case runs through gfw_undistort_frame and through a 2-frame gfw_undistort_clip (whose second frame joins the launch by its pointers alone), with the
specialised kernel (GFW_OPT_JIT 2) and the ahead-of-time one (0).  A tile is 128 x 16 luma pixels.  (Written for round 7's paired chroma store — a lane pair's U and V
samples as one store instruction, measured slower and removed: profiles/r07_row_memops.txt — whose cases these are.)"""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _oracle as O
from test_gpu_fullsize import _View

pytestmark = pytest.mark.gpu

FILL = 0x5A
# 8-bit 4:2:2 planar: three Luma8 planes, chroma halved across.  The render table has no such format (it converts YUV422P: rendering/mod.rs:641-649), so
# gyroflow_amd.formats does not list it; the library serves the plane list like any other
S.FRAME_FORMATS.setdefault("YUV422P", [("Luma8", (1, 1), [0], 255.0), ("Luma8", (2, 1), [1], 255.0), ("Luma8", (2, 1), [2], 255.0)])
_frames, _refs = {}, {}


def frames_of(fmt, w, h, pad=0, **kw):
    """two frames of one clip (cached: built once per shape), destination pitches widened by `pad` bytes"""
    key = (fmt, w, h, pad, repr(sorted(kw.items())))
    if key not in _frames:
        frs = [S.SyntheticFrame(fmt, w, h, seed=0x7A0 + 13 * j, timestamp_ms=1000.0 + 33.3 * j, pixels=False, **kw) for j in range(2)]
        for fr in frs:
            for pl in fr.planes:
                ow, oh, ostride = pl["out_size"]
                pl["out_size"] = (ow, oh, ostride + pad)
                pl["params"].output_stride = ostride + pad
        _frames[key] = frs
    return key, _frames[key]


def reference(key, j, fr, src):
    """the oracle's planes of frame j (computed once per shape, shared by the cases and left unchanged)"""
    if (key, j) not in _refs:
        _refs[(key, j)] = [np.array(p, copy=True) for p in O.run_frame(_View(fr, src))]
        for p in _refs[(key, j)]:
            p.setflags(write=False)
    return _refs[(key, j)]


def place(fr, layout, gap, dev):
    """destination planes of one frame -> ([plane views], [(whole allocation, [(offset, size) of the planes inside it])]), everything pre-filled"""
    import torch
    sizes = [pl["out_size"][2] * pl["out_size"][1] for pl in fr.planes]
    if layout == "sep":
        bufs = [torch.full((s + 512,), FILL, dtype=torch.uint8, device=dev) for s in sizes]          # (256 bytes of fill on either side of every plane)
        return [b[256:256 + s] for b, s in zip(bufs, sizes)], [(b, [(256, s)]) for b, s in zip(bufs, sizes)]
    order = {"uv": [0, 1, 2], "vu": [0, 2, 1]}[layout]
    off, cur = {}, 256
    for p in order:
        off[p] = cur
        cur = S.align(cur + sizes[p], 256) + gap
    buf = torch.full((cur,), FILL, dtype=torch.uint8, device=dev)
    return [buf[off[p]:off[p] + sizes[p]] for p in range(len(sizes))], [(buf, [(off[p], sizes[p]) for p in range(len(sizes))])]


def run(frames, layouts, jit, use_clip, gaps=(256, 256), checksums=False):
    """-> (per frame: source planes, destination planes, allocations as host arrays), backend, checksum words"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(frames)
    d_src = [fr.device_planes(dev) for fr in frames]
    placed = [place(fr, layouts[j], gaps[j], dev) for j, fr in enumerate(frames)]
    d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
    d_sums = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    params = [pl["params"] for pl in frames[0].planes]
    bufs = [[warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"], placed[j][0][p].data_ptr(), placed[j][0][p].numel(), pl["out_size"])
             for p, pl in enumerate(fr.planes)] for j, fr in enumerate(frames)]
    rows = frames[0].matrices.shape[0]
    be = warp.Backend(params[0], types[0], frames[0].model, frames[0].digital, bufs[0][0])
    try:
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        be.set_option(abi.OPT_JIT, jit)
        if checksums:
            be.set_frame_checksums(d_sums.data_ptr(), n)
        if use_clip:
            warp.ClipCall(be, bufs, params, types, [m.data_ptr() for m in d_mat], rows)()
        else:
            for j in range(n):
                warp.FrameCall(be, bufs[j], params, types, d_mat[j].data_ptr(), rows)()
        be.synchronize()
        backend = warp.last_backend()
        if checksums:
            be.set_frame_checksums(0, 0)
    finally:
        be.close()
    torch.cuda.synchronize(dev)
    out = []
    for j in range(n):
        out.append(([t.cpu().numpy() for t in d_src[j]], [t.cpu().numpy() for t in placed[j][0]], [(b.cpu().numpy(), spans) for b, spans in placed[j][1]]))
    return out, backend, [int(v) & 0xFFFFFFFFFFFFFFFF for v in d_sums.cpu().numpy()]


def check(key, frames, layouts=("sep", "sep"), gaps=(256, 256), what=""):
    for jit in (2, 0):
        for use_clip in (False, True):
            out, backend, _ = run(frames, layouts, jit, use_clip, gaps)
            tag = "%s: jit %d, %s (%s)" % (what, jit, "2-frame clip" if use_clip else "frame calls", backend)
            assert backend.endswith("_jit") == (jit == 2) and backend.startswith("yuv_fused"), tag
            for j, (src, dst, allocs) in enumerate(out):
                ref = reference(key, j, frames[j], src)
                for p, (a, b) in enumerate(zip(ref, dst)):                # every byte of the plane: pixels and row padding
                    bad = np.flatnonzero(a != b)
                    assert bad.size == 0, "%s, frame %d plane %d: %d bytes differ from the oracle, first at %d" % (tag, j, p, bad.size, bad[0])
                for whole, spans in allocs:                               # ... and whatever lies around the planes is untouched
                    outside = np.ones(whole.size, dtype=bool)
                    for off, size in spans:
                        outside[off:off + size] = False
                    assert np.all(whole[outside] == FILL), "%s, frame %d: bytes outside the planes were written" % (tag, j)


@pytest.mark.parametrize("fmt", ["YUV422P16LE", "YUV422P"])
def test_whole_tiles(fmt):
    """256 x 32: two tiles across, two down, every lane of every wave live"""
    key, frames = frames_of(fmt, 256, 32)
    check(key, frames, what=fmt)


@pytest.mark.parametrize("w,h", [(254, 16), (130, 18)])
def test_odd_chroma_width_and_partial_tiles(w, h):
    """chroma widths 127 and 65: the last tile's wave holds dead lanes; nothing may land beyond a row's end (the padding is compared with the oracle's)"""
    for fmt in ("YUV422P16LE", "YUV422P"):
        key, frames = frames_of(fmt, w, h)
        check(key, frames, what="%s %dx%d" % (fmt, w, h))


@pytest.mark.parametrize("fmt", ["YUV420P", "YUV444P16LE"])
def test_other_planar_subsamplings(fmt):
    key, frames = frames_of(fmt, 256, 32)
    check(key, frames, what=fmt)


def test_interleaved_chroma():
    key, frames = frames_of("NV12", 256, 32)
    check(key, frames, what="NV12")


@pytest.mark.parametrize("layouts,gaps", [
    (("uv", "uv"), (256, 256)),              # U before V in one allocation
    (("vu", "vu"), (256, 256)),              # V before U
    (("sep", "sep"), (256, 256)),            # separate allocations
    (("uv", "vu"), (256, 4096 + 64)),        # the two frames of a clip launch with different plane distances (and orders)
])
def test_plane_placement(layouts, gaps):
    """destination pitches padded by 64 bytes; the gaps between the planes of an allocation must keep their fill"""
    key, frames = frames_of("YUV422P16LE", 256, 32, pad=64)
    check(key, frames, layouts, gaps, what="planes %s" % (layouts,))


@pytest.mark.parametrize("bg", [0, 1])
def test_border_waves_beside_interior_waves(bg):
    """fov 2.0 brings the frame's border into the picture: waves that fail the interior vote (edge-aware stores, per lane) sit beside waves that pass it"""
    key, frames = frames_of("YUV422P16LE", 256, 32, fov=2.0, base_overrides={"background_mode": bg}, background_rgba=(0.25, 0.5, 0.75, 1.0))
    check(key, frames, what="background mode %d" % bg)


def test_checksum_flavour_adds_what_the_stored_bytes_add():
    """gfw_set_frame_checksums: each frame's word = the sum over its planes of the 64-bit words of the bytes WRITTEN (stride padding left out), from the oracle's bytes"""
    key, frames = frames_of("YUV422P16LE", 256, 32)
    for jit in (2, 0):
        for use_clip in (False, True):
            out, backend, sums = run(frames, ("uv", "sep"), jit, use_clip, checksums=True)
            for j, (src, dst, _) in enumerate(out):
                ref = reference(key, j, frames[j], src)
                want = 0
                for p, pl in enumerate(frames[j].planes):
                    ow, oh, ostride = pl["out_size"]
                    row_bytes = ow * pl["params"].bytes_per_pixel
                    body = np.zeros(S.align(ostride * oh, 8), np.uint8)
                    body[:oh * ostride].reshape(oh, ostride)[:, :row_bytes] = ref[p][:oh * ostride].reshape(oh, ostride)[:, :row_bytes]
                    want += int(body.view(np.uint64).sum(dtype=np.uint64))
                    assert np.array_equal(ref[p], dst[p]), "jit %d %s, frame %d plane %d" % (jit, backend, j, p)
                assert sums[j] == want & 0xFFFFFFFFFFFFFFFF, "jit %d, %s (%s), frame %d: %#x != %#x" % (jit, "clip" if use_clip else "frame calls", backend, j, sums[j], want & 0xFFFFFFFFFFFFFFFF)
