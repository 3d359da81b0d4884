"""TEST INFRASTRUCTURE: the zoom search's host statement (tests/_zoomstmt.py) extended with what a clip from a camera with stabiliser data and a per-frame lens
mesh adds — at_timestamp_for_points' shifts (frame_transform.rs:412-435) and the mesh handed to undistort_points (cpu_undistort.rs:712-760) — the statement clips of
those paths, their arguments for gfw_zoom_fovs_stab / gfw_build_matrices_batch_stab, and the host-interpreted kernels (tests/emu/emu_zoom_stab_driver.inc,
emu_matrices_stab_driver.inc).  Written from the cited Rust, independent of the device code; not part of the product package.

  point_shifts   frame_transform.rs:412-435: the scale is width / crop_w / pitch_x, height / crop_h / pitch_y (no framebuffer sign, no sensor-height flip: those
                 are the matrix path's); the spline position map_coord(y as f64, 0, height, crop_y, crop_y + crop_h) + offset with the point's own y as given, under
                 horizontal readout too; the roll (s.z / 1000).to_radians() as f32; an absent or unevaluable spline gives zeros.  Without rolling shutter points_iter
                 is the single point (0, 0): ONE shift at y = 0.  suppress_rotation 2 (`params.suppress_rotation && params.frame_readout_time == 0.0`): None.
  map_points     cpu_undistort.rs:752 `shift_per_point.as_ref().and_then(|v| v.get(index))`: with one shift only index 0 of each mapped set — outline point 0 and
                 point 0 of every refinement — is shifted, every other point is mapped WITHOUT a shift (which is not a shift of zeros: `x - c - 0 + 0` followed by
                 `1 * x - 0 * y + c` rounds).  The oracle's undistort_points indexes shifts like rotations (a row past the count falls back to row 0), so that form
                 is two oracle calls: point 0 with its shift, the others with none.

Spline amplitudes (stab_data): IBIS x / y 20 sensor units, OIS x / y 8, roll 100 (0.1 degree) on a 6000 x 3376 sensor cropped to 5760 x 2700 with pitch 3 — at
320 x 180 that is at most 0.37 / 0.44 px of IBIS shift, 0.15 / 0.18 px of OIS shift and 0.32 px of roll at the corner: about a pixel together, well inside the
3 % band of tests/test_zoom_stab_statement.py (4.8 px horizontally, 2.7 px vertically), which the no-rolling-shutter form needs — it shifts one outline point only,
while the render shifts the whole frame."""
import copy
import ctypes as C
import math

import numpy as np

from gyroflow_amd import abi, warp
import _emu
import _hoststmt as H
import _oracle as O
import _zoomcase as ZC
import _zoomstmt as Z
from test_gpu_lens_models import synthetic_mesh

f32 = np.float32
IBIS_XY, OIS_XY, ROLL = 20.0, 8.0, 100.0


def stab_data(size, k, evaluable=True):
    """camera_stab_data[frame k] as the dict Backend.build_matrices takes (19 control points over the sensor's readout, another phase per frame).
    evaluable=False: every position lies past the sensor — both splines answer None, the shift is (0, 0, 0, 0, 0)."""
    pos = np.linspace(-200.0, 3400.0, 19) + (0.0 if evaluable else 50000.0)
    ph = 0.37 * k
    ibis = np.stack([pos, IBIS_XY * np.sin(pos * 0.004 + ph), -IBIS_XY * np.cos(pos * 0.003 - ph), ROLL * np.sin(pos * 0.002 + 0.4 + ph)], axis=1)
    ois = np.stack([pos, OIS_XY * np.cos(pos * 0.005 - ph), OIS_XY * np.sin(pos * 0.006 + ph), np.zeros_like(pos)], axis=1)
    return {"offset": 12.5, "sensor_size": (6000.0, 3376.0), "crop_area": (120.0, 338.0, 5760.0, 2700.0), "pixel_pitch": (3.0, 3.0),
            "width": float(size[0]), "height": float(size[1]), "ibis": ibis, "ois": ois}


class StabClip(Z.Clip):
    """A statement clip with per-frame stabiliser data and meshes.
    stab: None; "all"; "mixed" — frames 2, 5, 8, ... have no camera_stab_data entry and frame 4's splines cannot be evaluated (a shift of zeros).
    mesh: None; "mesh" (the bivariate spline); "fpd" (the focal-plane-distortion block alone); "both".  Frames 0..11 name ONE array, frames 12.. another,
    frame 7 none.  suppress_mode: gfw_zoom_frame.suppress_rotation (0, 1, 2)."""

    def __init__(self, name, stab="all", mesh=None, suppress_mode=0, **kw):
        Z.Clip.__init__(self, name, suppress=suppress_mode != 0, **kw)
        self.stab, self.mesh, self.suppress_mode = stab, mesh, suppress_mode
        self._stabs = [self._stab_at(k) for k in range(len(self.timestamps))]
        self._meshes = None
        if mesh:
            a = synthetic_mesh(self.size[0], self.size[1], with_fpd=mesh in ("fpd", "both"), with_mesh=mesh in ("mesh", "both")).astype(np.float64)
            b = a.copy()
            o = int(b[0])
            if b[0] > 10.0:
                b[9 + 81 * 2:9 + 81 * 2 + 81 * 8] *= 1.0 + 1e-3                                    # another frame's coefficients
            if mesh in ("fpd", "both"):
                b[o + 4:o + 20] *= -1.5
            self._meshes = [None if k == 7 else (a if k < 12 else b) for k in range(len(self.timestamps))]

    def _stab_at(self, k):
        if self.stab is None or (self.stab == "mixed" and k % 3 == 2):
            return None
        return stab_data(self.size, k, evaluable=not (self.stab == "mixed" and k == 4))

    def with_mode(self, suppress_mode=0, readout=None, horizontal=None):
        """the same clip under another suppress_rotation / readout"""
        c = copy.copy(self)
        c.suppress_mode, c.suppress = suppress_mode, suppress_mode != 0
        if readout is not None:
            c.readout = float(readout)
        if horizontal is not None:
            c.horizontal = horizontal
        return c

    def stabs(self):
        """[dict or None per frame], or None: the clip has no camera_stab_data"""
        return None if self.stab is None else list(self._stabs)

    def meshes(self):
        return None if self._meshes is None else list(self._meshes)


def stab_clips():
    P = Z.physical_lens
    return [
        StabClip("shifts-r0", stab="mixed"),
        StabClip("shifts-r12", stab="mixed", readout=12.0, center=(0.04, -0.03), out=(240, 180)),
        StabClip("shifts-r12-horizontal", stab="all", readout=12.0, horizontal=True),
        StabClip("shifts-r12-l0.6", stab="mixed", readout=12.0, lca=0.6),
        StabClip("shifts-r0-l0.6", stab="all", lca=0.6),
        StabClip("mesh-r12", stab=None, mesh="mesh", readout=12.0),
        StabClip("fpd-r0", stab=None, mesh="fpd"),
        StabClip("all-r12-sony", stab="mixed", mesh="both", readout=12.0, lens=P("sony", (320, 180)), seed=13),
        StabClip("all-r0-poly5", stab="mixed", mesh="both", lens=P("poly5", (320, 180)), seed=13),
        StabClip("all-r12-digital", stab="mixed", mesh="both", readout=12.0, lca=0.6, digital="gopro_superview", digital_params=[], out=(240, 180)),
        StabClip("all-r0-keyframed", stab="mixed", mesh="both", lca=0.9, center=(0.01, -0.01), keyframed=True),
    ]


PURPOSE = ["shifts-r0", "shifts-r12", "shifts-r12-horizontal", "shifts-r12-l0.6", "shifts-r0-l0.6"]       # IBIS/OIS splines with and without rolling shutter


# ------------------------------------------------------------------------------------------------ frame_transform.rs:412-435
def map_coord(x, in_min, in_max, out_min, out_max):
    return (x - in_min) * (out_max - out_min) / (in_max - in_min) + out_min                             # util.rs:144-147


def point_shifts(clip, stab, pts):
    """-> None, or [n][5] f32 (sx, sy, angle_rad, ox, oy): one row per point with rolling shutter, ONE row without."""
    if stab is None or clip.suppress_mode == 2:                                                            # :412 `camera_stab_data.get(frame)`; :433-435
        return None
    w, h = clip.size
    ca, pp = stab["crop_area"], stab["pixel_pitch"]
    is_scale = (float(w) / float(ca[2]) / float(pp[0]), float(h) / float(ca[3]) / float(pp[1]))
    out = []
    for _x, y in (pts if abs(clip.readout) > 0.0 else [(0.0, 0.0)]):                                      # :389 points_iter
        ys = map_coord(float(y), 0.0, float(h), float(ca[1]), float(ca[1]) + float(ca[3]))
        s = H.catmull_rom_at(stab["ibis"], ys + stab["offset"])
        o = H.catmull_rom_at(stab["ois"], ys + stab["offset"])
        s = np.zeros(3) if s is None else s                                                                 # unwrap_or_default()
        o = np.zeros(3) if o is None else o
        ra = float(s[2]) / 1000.0
        out.append([f32(float(s[0]) * is_scale[0]), f32(float(s[1]) * is_scale[1]), f32(ra * (math.pi / 180.0)), f32(float(o[0]) * is_scale[0]), f32(float(o[1]) * is_scale[1])])
    return np.array(out, dtype=np.float32)


def mapper_for(clip, k, rotation=None, perturb=None, shift_every_point=False, points_fn=None):
    """map_points of frame k (see _zoomstmt.mapper_for for rotation / perturb).  shift_every_point: NOT the reference — a frame without rolling shutter hands its one
    shift to every point; what the index-0 case of the tests shows the result to differ from.  points_fn: the point map in the oracle's place, called as
    points_fn(kernel_params, rotations, points, shifts, mesh) with one rotation (and shift) row per point — the route gfw_zoom_fovs_stab replaces hands it to
    gfw_undistort_points."""
    kp = clip.kernel_params(k)
    stab = clip._stabs[k] if clip.stab is not None else None
    mesh = clip._meshes[k] if clip._meshes is not None else None
    cache = {}
    if perturb is not None and clip.suppress:
        perturb = None
    once = perturb.integers(-2, 3, (1, 9)).astype(np.int32) if perturb is not None and clip.readout == 0.0 else None

    def undistort(arr, rot, shifts):
        if points_fn is not None:
            return points_fn(kp, np.ascontiguousarray(rot), arr, shifts, mesh)
        return O.undistort_points(kp, clip.model, clip.digital, np.ascontiguousarray(rot), points=arr, shifts=shifts, index_mode=abi.POINT_INDEX_PER_POINT, mesh=mesh)

    def map_points(pass_index, pts):
        arr = np.array(pts, dtype=np.float32).reshape(-1, 2)
        if rotation is not None:
            assert clip.readout == 0.0
            rot = np.repeat(np.asarray(rotation, dtype=np.float32).reshape(1, 9), len(arr), 0)
        else:
            key = arr.tobytes()
            if key not in cache:
                cache[key] = Z.point_rotations(clip, pts, k)
            rot = cache[key]
            if rot.shape[0] == 1:
                rot = np.repeat(rot, len(arr), 0)
        if perturb is not None:
            delta = once if once is not None else perturb.integers(-2, 3, rot.shape).astype(np.int32)
            rot = np.where(rot == 0.0, rot, (rot.view(np.int32) + delta).view(np.float32))
        sh = point_shifts(clip, stab, pts)
        if sh is None:
            o = undistort(arr, rot, None)
        elif len(sh) == len(arr) and abs(clip.readout) > 0.0:
            o = undistort(arr, rot, sh)
        elif shift_every_point:
            o = undistort(arr, rot, np.repeat(sh[:1], len(arr), 0))
        else:                                                                                               # shift_per_point.get(index): index 0 only
            o = np.concatenate([undistort(arr[:1], rot[:1], sh[:1]), undistort(arr[1:], rot[1:], None)])
        return [(f32(x), f32(y)) for x, y in o]
    return map_points


def frame_fov(clip, k, rotation=None, perturb=None, shift_every_point=False, points_fn=None):
    return Z.find_fov(mapper_for(clip, k, rotation, perturb, shift_every_point, points_fn), clip.size[0], clip.size[1], clip.out, clip.margin, clip.center_at(k))


def clip_fovs(clip, given_rotations=False, perturb=None, shift_every_point=False, frames=None):
    """find_fov of every frame (or of `frames`) -> (fov_minimal f64, debug polygons [n][120][2] f64)"""
    fovs, dbg = [], []
    for k in (range(len(clip.timestamps)) if frames is None else frames):
        f, d = frame_fov(clip, k, Z.frame_rotation(clip, k) if given_rotations else None, perturb, shift_every_point)
        fovs.append(f)
        dbg.append(d)
    return np.array(fovs, dtype=np.float64), np.array(dbg, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the render of the purpose test
def stab_terms(clip, k, rows):
    """m[9..13] of frame k's rows (frame_transform.rs:270-289) from the matrix builder's statement, or None: the frame has no stabiliser data"""
    stab = clip._stabs[k] if clip.stab is not None else None
    if stab is None:
        return None
    org, smoothed = clip.tracks
    m = H.row_matrices_from_tracks(org, smoothed, clip.new_k(), clip.timestamps[k], clip.readout, rows, clip.size[0] if clip.horizontal else clip.size[1], stab=stab)
    return m[:, 9:14]


def background_pixels(clip, k, fov):
    """_zoomcase.background_pixels with the frame's IBIS/OIS terms in its rows: the frame rendered by the oracle at this fov, twice, with two background values"""
    t = ZC.frame_transform(clip, k, fov)
    terms = stab_terms(clip, k, t.matrices.shape[0])
    if terms is not None:
        t.matrices[:, 9:14] = terms
    outs = []
    for bg in (0.0, 1.0):
        fr = ZC.render_frame(clip, k, fov, bg, transform=t)
        pl = fr.planes[0]
        dst = pl["dst"].copy()
        assert O.undistort_image(pl["src"], pl["size"], dst, pl["out_size"], pl["params"], pl["pixel_type"], fr.model, fr.digital, fr.matrices) == 1
        outs.append(dst)
    return int(np.count_nonzero(outs[0] != outs[1]))


# ------------------------------------------------------------------------------------------------ arguments of the entry / the interpreted kernel
def inputs(clip, given_rotations=False, tile=1):
    """-> (KernelParams, abi.ZoomSearch, frames, rotations or None, stabs [dict or None] or None, meshes [array or None] or None); tile: the frames repeated"""
    kp, search, frames, rot = ZC.inputs(clip, given_rotations, tile)
    for f in frames:
        f.suppress_rotation = clip.suppress_mode
    stabs, meshes = clip.stabs(), clip.meshes()
    return kp, search, frames, rot, (stabs * tile if stabs is not None else None), (meshes * tile if meshes is not None else None)


_zlib = None


def emu_zoom_fovs(params, model, digital, search, frames, rotations=None, stabs=None, meshes=None, tracks=None, offsets=None, duration_ms=1.0):
    """gfw_zoom_fovs_stab through the host-interpreted gfw_zoom_stab_kernel<MODEL> -> (fov_minimal [n] f64, debug polygons [n][120][2] f64)"""
    global _zlib
    if _zlib is None:
        L = C.CDLL(_emu.build({}, "", top="gfw_zoom.hip", n_asm=2, driver="emu_zoom_stab_driver.inc", extra_flags=()))
        vp, i32 = C.c_void_p, C.c_int
        L.gfw_emu_zoom_stab.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, C.c_double, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        _zlib = L
    n = len(frames)
    com = _emu.common_for(_emu._Lenses(model, digital), params)
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data if a.size else None
    if tracks is not None:
        (ot, oq), (st, sq) = tracks
        targs = [arr(ot, np.int64), arr(oq, np.float64), len(ot), arr(st, np.int64), arr(sq, np.float64), len(st)]
    else:
        targs = [None, None, 0, None, None, 0]
    targs += [arr(offsets[0], np.int64), arr(offsets[1], np.float64), len(offsets[0])] if offsets else [None, None, 0]
    fov, dbg = np.zeros(n, dtype=np.float64), np.zeros((n, 120, 2), dtype=np.float64)
    rp = arr(np.asarray(rotations, dtype=np.float32).reshape(-1, 9), np.float32) if rotations is not None else None
    sp = mp = lp = None                                                          # the entry point's own arguments (warp.Backend.zoom_fovs_stab makes them the same way)
    if stabs is not None:
        sp, held = warp.frame_stab_table(stabs)
        keep.append(held)
    if meshes is not None:
        mp, lp, held = warp.frame_mesh_table(meshes)
        keep.append(held)
    rc = _zlib.gfw_emu_zoom_stab(C.cast(C.byref(params), C.c_void_p), C.cast(C.byref(com), C.c_void_p), *targs, float(duration_ms),
                                 C.cast(C.byref(search), C.c_void_p), C.cast(frames, C.c_void_p), n, rp, fov.ctypes.data, dbg.ctypes.data, sp, mp, lp)
    assert rc == 0, "gfw_emu_zoom_stab -> %d" % rc
    return fov, dbg


def emu_clip_fovs(clip, given_rotations=False):
    """the clip through the interpreted kernel: caller-given rotations (the statement's own, readout 0), or rotations from the clip's tracks"""
    kp, search, frames, rot, stabs, meshes = inputs(clip, given_rotations)
    if given_rotations:
        return emu_zoom_fovs(kp, clip.model, clip.digital, search, frames, rotations=rot, stabs=stabs, meshes=meshes)
    return emu_zoom_fovs(kp, clip.model, clip.digital, search, frames, stabs=stabs, meshes=meshes, tracks=clip.tracks, offsets=clip.sync_offsets, duration_ms=clip.duration_ms)


def emu_build_matrices_stab(org, smoothed, timings, stabs, rows, offsets=None, duration_ms=1.0):
    """gfw_build_matrices_batch_stab through the host-interpreted gfw_build_matrices_stab_kernel: timings = ctypes array of abi.FrameTiming, stabs = [dict or None]
    -> float32 [frames][rows][16]"""
    lib = C.CDLL(_emu.build({}, "", top="gfw_matrices.hip", n_asm=2, driver="emu_matrices_stab_driver.inc", extra_flags=()))
    n = len(timings)
    ot, oq = np.ascontiguousarray(org[0], dtype=np.int64), np.ascontiguousarray(org[1], dtype=np.float64)
    st, sq = np.ascontiguousarray(smoothed[0], dtype=np.int64), np.ascontiguousarray(smoothed[1], dtype=np.float64)
    fts = np.ascontiguousarray(offsets[0] if offsets else [], dtype=np.int64)
    fms = np.ascontiguousarray(offsets[1] if offsets else [], dtype=np.float64)
    out = np.zeros((n, rows, 16), dtype=np.float32)
    table, keep = warp.frame_stab_table(stabs)
    lib.gfw_emu_build_matrices_stab.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                                C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    rc = lib.gfw_emu_build_matrices_stab(ot.ctypes.data, oq.ctypes.data, len(ot), st.ctypes.data, sq.ctypes.data, len(st),
                                         fts.ctypes.data if len(fts) else None, fms.ctypes.data if len(fts) else None, len(fts), float(duration_ms),
                                         C.cast(timings, C.c_void_p), n, rows, out.ctypes.data, rows * 16, C.cast(table, C.c_void_p))
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------------ the batch of gfw_build_matrices_batch_stab's tests
def batch_case(n, w, h, nk, readout_ms=16.0):
    """`n` frames mixing NULL and real stabiliser entries (every third frame has none), both framebuffer orientations and suppress_rotation 0 / 1 / 2
    -> (ctypes array of abi.FrameTiming, [dict or None])"""
    from test_gpu_matrix_builder import _stab
    timings = (abi.FrameTiming * n)()
    nkf = np.asarray(nk, dtype=np.float64).reshape(9)
    stabs = []
    for k in range(n):
        t = timings[k]
        t.timestamp_ms, t.per_frame_time_offset_ms, t.frame_readout_time_ms = 1000.3 + 13.7 * k, 0.05 * (k % 4), readout_ms
        for i in range(9):
            t.new_k[i] = nkf[i]
        t.video_rotation_deg, t.rows, t.readout_dim = 0.0, h, h
        t.framebuffer_inverted = (k // 2) % 2
        t.suppress_rotation = (0, 0, 1, 0, 2, 0, 0)[k % 7]
        st = None
        if k % 3 != 1:
            st = _stab(w, h)
            st["ibis"] = np.asarray(st["ibis"], dtype=np.float64).copy()
            st["ibis"][:, 1:] *= 1.0 + 0.11 * k
            st["offset"] = 12.5 + k
        stabs.append(st)
    return timings, stabs
