"""Thin ctypes driver over the C ABI (include/gfwarp.h).

``Backend`` plays the role of the reference's ``OclWrapper`` / ``WgpuWrapper`` objects
(src/core/gpu/opencl.rs:178,330): construct once per (size, pixel type, lens model) key, then call
``undistort_image`` per plane or ``undistort_frame`` per frame.  All pixel work happens in
libgfwarp.so on the GPU; this module only marshals pointers.
"""
import ctypes as C

import numpy as np

from . import abi


class GfwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (abi.ERRORS.get(code, "?"), code, msg))
        self.code = code
        self.name = abi.ERRORS.get(code, "?")


def _desc(d, size, kind, ptr, nbytes, rect=None, rotation=None):
    d.width, d.height, d.stride = size
    d.has_rect = 1 if rect is not None else 0
    if rect is not None:
        for i in range(4):
            d.rect[i] = rect[i]
    d.has_rotation = 1 if rotation is not None else 0
    d.rotation = rotation or 0.0
    d.kind = kind
    d.data = ptr
    d.len = nbytes


def host_buffers(src, in_size, dst, out_size, in_rect=None, out_rect=None, in_rot=None, out_rot=None):
    """``Buffers`` over two numpy uint8 arrays (BufferSource::Cpu)."""
    b = abi.Buffers()
    _desc(b.input, in_size, abi.BUF_HOST, src.ctypes.data, src.nbytes, in_rect, in_rot)
    _desc(b.output, out_size, abi.BUF_HOST, dst.ctypes.data, dst.nbytes, out_rect, out_rot)
    return b


def device_buffers(src_ptr, src_len, in_size, dst_ptr, dst_len, out_size, in_rect=None, out_rect=None):
    """``Buffers`` over raw HIP device pointers (the CUDABuffer analogue)."""
    b = abi.Buffers()
    _desc(b.input, in_size, abi.BUF_HIP_DEVICE, src_ptr, src_len, in_rect)
    _desc(b.output, out_size, abi.BUF_HIP_DEVICE, dst_ptr, dst_len, out_rect)
    return b


_last_backend = ""


def frame_stab(stab):
    """abi.FrameStab of dict(offset, sensor_size, crop_area, pixel_pitch, width, height, ibis=[n][4], ois=[n][4]) -> (struct, the arrays it points into)"""
    st = abi.FrameStab()
    st.offset = stab["offset"]
    st.sensor_size[0], st.sensor_size[1] = stab["sensor_size"]
    for i in range(4):
        st.crop_area[i] = stab["crop_area"][i]
    st.pixel_pitch[0], st.pixel_pitch[1] = stab["pixel_pitch"]
    st.width, st.height = stab["width"], stab["height"]
    ibis = np.ascontiguousarray(stab["ibis"], dtype=np.float64).reshape(-1, 4)
    ois = np.ascontiguousarray(stab["ois"], dtype=np.float64).reshape(-1, 4)
    st.ibis_count, st.ois_count = ibis.shape[0], ois.shape[0]
    st.ibis, st.ois = ibis.ctypes.data, ois.ctypes.data
    return st, (ibis, ois)


def frame_stab_table(stabs):
    """[dict or None per frame] -> (ctypes array of gfw_frame_stab pointers, NULL where None; what it points into)"""
    table, keep = (C.c_void_p * max(len(stabs), 1))(), []
    for k, stab in enumerate(stabs):
        if stab is not None:
            keep.append(frame_stab(stab))
            table[k] = C.addressof(keep[-1][0])
    return table, keep


def frame_mesh_table(meshes):
    """[float64 mesh or None per frame] -> (ctypes arrays of pointers and lengths as gfw_zoom_fovs_stab takes them, NULL / 0 where None; what they point into).
    Frames that name the SAME array object share one conversion, hence one pointer.  Public like frame_stab_table beside it: the interpreter tier of the tests
    hands the entry point's own arguments to the host-interpreted kernels."""
    n = max(len(meshes), 1)
    mp, lp, held = (C.c_void_p * n)(), (C.c_size_t * n)(), {}
    for k, m in enumerate(meshes):
        if m is None or len(m) == 0:
            continue
        if id(m) not in held:
            held[id(m)] = np.ascontiguousarray(m, dtype=np.float64)
        mp[k], lp[k] = held[id(m)].ctypes.data, held[id(m)].size
    return mp, lp, held


def _matrix_arg(matrices, matrix_count=None):
    """a frame's rows as numpy [rows][14] f32, or a device pointer (GFW_OPT_MATRICES_ON_DEVICE) with its row count -> (pointer, rows, the array to keep alive)"""
    if isinstance(matrices, np.ndarray):
        m = np.ascontiguousarray(matrices, dtype=np.float32)
        return m.ctypes.data, m.shape[0], m
    return matrices, matrix_count, None


def _mesh_arg(mesh, dtype=np.float32):
    """None, an empty or a lens mesh -> (pointer or None, values, the array to keep alive)"""
    if mesh is None or not len(mesh):
        return None, 0, None
    m = np.ascontiguousarray(mesh, dtype=dtype)
    return m.ctypes.data, m.size, m


def _frames_arg(frames, shape):
    """u8 gray planes as numpy [n][height][stride], or a device pointer (int) with `shape` = (n, height, stride) -> (pointer or None, on-device flag,
    (n, height, stride), the array to keep alive)"""
    if isinstance(frames, (int, np.integer)):
        return int(frames), 1, tuple(shape), None
    keep = np.ascontiguousarray(frames, dtype=np.uint8)
    assert keep.ndim == 3, "frames: [n][height][stride]"
    return (keep.ctypes.data if keep.size else None), 0, keep.shape, keep


def last_backend():
    return _last_backend


class Backend:
    def __init__(self, params, pixel_type, model, digital, buffers, drawing_len=0):
        self.lib = abi.load_library()
        pid = abi.PIXEL_TYPES[pixel_type][0] if isinstance(pixel_type, str) else pixel_type
        self.ctx = self.lib.gfw_create(C.byref(params), pid, model, digital, C.byref(buffers), drawing_len)
        if not self.ctx:
            raise GfwError(-100, self.lib.gfw_last_error().decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gfw_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def _check(self, rc):
        global _last_backend
        if rc != 0:
            raise GfwError(rc, self.lib.gfw_last_error().decode())
        _last_backend = self.lib.gfw_last_backend(self.ctx).decode()

    @staticmethod
    def last_backend_of(be):
        """gfw_last_backend of this context (the module-level last_backend() names whichever context was called last)."""
        return be.lib.gfw_last_backend(be.ctx).decode()

    def set_option(self, opt, value):
        self._check(self.lib.gfw_set_option(self.ctx, opt, value))

    def set_stream(self, stream_ptr):
        self._check(self.lib.gfw_set_stream(self.ctx, stream_ptr))

    def get_stream(self):
        """hipStream_t the context enqueues on (an int), after whatever it holds for a frame or a launch has been enqueued (gfw_get_stream flushes)."""
        return self.lib.gfw_get_stream(self.ctx)

    def set_frame_checksums(self, d_sums_ptr, count):
        """From now on frame k submitted on the context adds the checksum of the bytes it writes to the device word d_sums_ptr[k % count] (gfw_set_frame_checksums);
        (0, 0) turns it off."""
        self._check(self.lib.gfw_set_frame_checksums(self.ctx, d_sums_ptr, count))

    def jit_status(self):
        """(state, compile milliseconds, compiler log) of the context's run-time specialised kernel; state 0 none / unavailable,
        1 compiling, 2 ready, 3 failed (gfw_jit_status)."""
        ms, log = C.c_double(0.0), C.create_string_buffer(4096)
        st = self.lib.gfw_jit_status(self.ctx, C.byref(ms), log, 4096)
        return st, ms.value, log.value.decode(errors="replace")

    def get_profile_frames(self, reset=True):
        """(kernel milliseconds, launches, frames those launches covered) since the last reset (needs OPT_PROFILE)."""
        ms, n, f = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.gfw_get_profile_frames(self.ctx, C.byref(ms), C.byref(n), C.byref(f), 1 if reset else 0))
        return ms.value, n.value, f.value

    def get_profile(self, reset=True):
        """(kernel milliseconds, launches) accumulated since the last reset (needs OPT_PROFILE)."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        self._check(self.lib.gfw_get_profile(self.ctx, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def get_audit(self, reset=False):
        """First-pass audit: (certified, certified_but_wrong, queued, queue_overflow, max |approx - exact| in pixels)."""
        arr = (C.c_ulonglong * 8)()
        self._check(self.lib.gfw_get_audit(self.ctx, C.byref(arr), 1 if reset else 0))
        gap = float(np.array([int(arr[4]) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
        return int(arr[0]), int(arr[1]), int(arr[2]), int(arr[3]), gap

    def get_audit_full(self, reset=False):
        """All audit words by name (first pass + address audit)."""
        arr = (C.c_ulonglong * 8)()
        self._check(self.lib.gfw_get_audit(self.ctx, C.byref(arr), 1 if reset else 0))
        gap = float(np.array([int(arr[4]) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
        return {"certified1": int(arr[0]), "certified1_wrong": int(arr[1]), "queued1": int(arr[2]), "queue_overflow": int(arr[3]),
                "pass1_gap_px": gap, "out_of_range": int(arr[5]),
                "pass1_eps_px": float(np.array([int(arr[6]) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])}

    def set_quaternion_tracks(self, org, smoothed):
        """Upload (timestamps_us int64, quaternions f64[n,4]) tracks once per clip (device matrix builder)."""
        ot, oq = np.ascontiguousarray(org[0], dtype=np.int64), np.ascontiguousarray(org[1], dtype=np.float64)
        st, sq = np.ascontiguousarray(smoothed[0], dtype=np.int64), np.ascontiguousarray(smoothed[1], dtype=np.float64)
        self._check(self.lib.gfw_set_quaternion_tracks(self.ctx, ot.ctypes.data, oq.ctypes.data, len(ot), st.ctypes.data, sq.ctypes.data, len(st)))

    def set_sync_offsets(self, duration_ms, timestamps_us=(), offsets_ms=()):
        """The clip's gyro/video sync offsets (GyroSource.offsets_adjusted) and duration (gyro_source/mod.rs:857-860)."""
        ts = np.ascontiguousarray(timestamps_us, dtype=np.int64)
        ov = np.ascontiguousarray(offsets_ms, dtype=np.float64)
        assert ts.shape == ov.shape
        self._check(self.lib.gfw_set_sync_offsets(self.ctx, float(duration_ms), ts.ctypes.data if len(ts) else None, ov.ctypes.data if len(ts) else None, len(ts)))

    def build_matrices(self, nk, timestamp_ms, frame_readout_time_ms, rows, readout_dim, video_rotation_deg=0.0,
                       framebuffer_inverted=False, per_frame_offset_ms=0.0, out_ptr=None, suppress_rotation=0, stab=None):
        """Build one frame's packed rows on the device; returns the device pointer (context-owned unless out_ptr given).
        stab: None or dict(offset, sensor_size, crop_area, pixel_pitch, width, height, ibis=[n][4], ois=[n][4])."""
        t = abi.FrameTiming()
        t.timestamp_ms, t.per_frame_time_offset_ms, t.frame_readout_time_ms = timestamp_ms, per_frame_offset_ms, frame_readout_time_ms
        for i, v in enumerate(np.asarray(nk, dtype=np.float64).reshape(9)):
            t.new_k[i] = v
        t.video_rotation_deg, t.rows, t.readout_dim = video_rotation_deg, rows, readout_dim
        t.framebuffer_inverted = 1 if framebuffer_inverted else 0
        t.suppress_rotation = int(suppress_rotation)
        ptr = C.c_void_p(0)
        if stab is None:
            self._check(self.lib.gfw_build_matrices(self.ctx, C.byref(t), out_ptr, C.byref(ptr)))
            return ptr.value
        st, _keep = frame_stab(stab)
        self._check(self.lib.gfw_build_matrices_stab(self.ctx, C.byref(t), C.byref(st), out_ptr, C.byref(ptr)))
        return ptr.value

    def build_matrices_batch(self, nk, timestamps_ms, frame_readout_time_ms, rows, readout_dim, video_rotation_deg=0.0,
                             framebuffer_inverted=False, per_frame_offset_ms=0.0, stabs=None, suppress_rotation=0):
        """Tables of several upcoming frames in one launch (gfw_build_matrices_batch); returns the device pointers.
        stabs: None, or one entry per frame — None or the dict build_matrices takes — (gfw_build_matrices_batch_stab).
        framebuffer_inverted / suppress_rotation: one value, or one per frame."""
        n = len(timestamps_ms)
        arr = (abi.FrameTiming * n)()
        nkf = np.asarray(nk, dtype=np.float64).reshape(9)
        per_frame = lambda v, k: v[k] if isinstance(v, (list, tuple)) else v
        for k, ts in enumerate(timestamps_ms):
            t = arr[k]
            t.timestamp_ms, t.per_frame_time_offset_ms, t.frame_readout_time_ms = ts, per_frame_offset_ms, frame_readout_time_ms
            for i in range(9):
                t.new_k[i] = nkf[i]
            t.video_rotation_deg, t.rows, t.readout_dim = video_rotation_deg, rows, readout_dim
            t.framebuffer_inverted = 1 if per_frame(framebuffer_inverted, k) else 0
            t.suppress_rotation = int(per_frame(suppress_rotation, k))
        ptrs = (C.c_void_p * n)()
        if stabs is None:
            self._check(self.lib.gfw_build_matrices_batch(self.ctx, arr, n, ptrs))
        else:
            assert len(stabs) == n
            table, _keep = frame_stab_table(stabs)
            self._check(self.lib.gfw_build_matrices_batch_stab(self.ctx, arr, table, n, ptrs))
        return [p for p in ptrs]

    def stmap_undistort(self, params, matrices, width, height, mesh=None, fill=None):
        """STMap 'undist' coordinates (stmap.rs:87-109) as a float32 array [height][width][2].  Where the projection is None an element keeps what the
        array started from: the 32-bit pattern ``fill`` (default 0, what parallel_exr leaves)."""
        m = np.ascontiguousarray(matrices, dtype=np.float32)
        coords = np.full((height, width, 2), fill or 0, dtype=np.uint32).view(np.float32)
        meshp, meshn, _mesh = _mesh_arg(mesh)
        self._check(self.lib.gfw_stmap_undistort(self.ctx, C.byref(params), m.ctypes.data, m.shape[0], meshp, meshn, width, height, coords.ctypes.data, 0))
        return coords

    def undistort_points(self, params, rotations, points=None, grid=None, shifts=None, index_mode=0, mesh=None):
        """Inverse point map (cpu_undistort.rs:652-858, lens_correction_amount == 1).

        ``points``: [n][2] float32, or None with ``grid=(w, h)`` for the pixel grid.  ``rotations``: [count][9] float32
        (`new_k * R` row-major), ``shifts``: None or [count][5], ``mesh``: None or float64 mesh data.
        Returns float32 [n][2] (or [h][w][2] for a grid)."""
        rot = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1, 9)
        if points is not None:
            pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
            n, gw, pp, shape = pts.shape[0], 0, pts.ctypes.data, (pts.shape[0], 2)
        else:
            gw, gh = grid
            n, pp, shape = gw * gh, None, (gh, gw, 2)
        out = np.zeros(shape, dtype=np.float32)
        sp = None
        if shifts is not None:
            shifts = np.ascontiguousarray(shifts, dtype=np.float32).reshape(-1, 5)
            assert shifts.shape[0] == rot.shape[0]
            sp = shifts.ctypes.data
        meshp, meshn, _mesh = _mesh_arg(mesh, np.float64)
        self._check(self.lib.gfw_undistort_points(self.ctx, C.byref(params), pp, n, gw, rot.ctypes.data, rot.shape[0], sp,
                                                  index_mode, meshp, meshn, out.ctypes.data, 0))
        return out

    def zoom_fovs(self, params, search, frames, rotations=None, debug=False, out_ptr=None, debug_ptr=None):
        """FovIterative::find_fov of every frame of a clip in one device call (gfw_zoom_fovs).

        ``params``: the KernelParams `undistort_points` builds; ``search``: abi.ZoomSearch; ``frames``: a ctypes array (or list) of
        abi.ZoomFrame; ``rotations``: None (rotations from the tracks of set_quaternion_tracks) or [n][9] float32, one `new_k * R` per frame.
        Returns float64 [n] — with ``debug`` also the first round's polygon, float64 [n][120][2] — or, with ``out_ptr`` (a device pointer to n
        doubles; ``debug_ptr``: None or a device pointer to n * 240 doubles), None: the results stay on the device, in order on the stream."""
        n = len(frames)
        arr = frames if isinstance(frames, C.Array) else (abi.ZoomFrame * max(n, 1))(*frames)
        rp = None
        if rotations is not None:
            rot = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1, 9)
            assert rot.shape[0] == n
            rp = rot.ctypes.data
        if out_ptr is not None:
            self._check(self.lib.gfw_zoom_fovs(self.ctx, C.byref(params), C.byref(search), C.cast(arr, C.c_void_p), n, rp, out_ptr, debug_ptr, 1))
            return None
        fov = np.zeros(n, dtype=np.float64)
        dbg = np.zeros((n, abi.ZOOM_RECT_POINTS, 2), dtype=np.float64) if debug else None
        self._check(self.lib.gfw_zoom_fovs(self.ctx, C.byref(params), C.byref(search), C.cast(arr, C.c_void_p), n, rp, fov.ctypes.data,
                                           dbg.ctypes.data if debug else None, 0))
        return (fov, dbg) if debug else fov

    def zoom_fovs_stab(self, params, search, frames, rotations=None, stabs=None, meshes=None, debug=False, out_ptr=None, debug_ptr=None):
        """zoom_fovs for clips with stabiliser data and lens meshes (gfw_zoom_fovs_stab).  ``stabs``: None, or one entry per frame —
        None (camera_stab_data has no entry for the frame) or the dict build_matrices takes; ``meshes``: None, or one entry per frame — None
        or the frame's float64 distorting mesh (frames that name the SAME array object consecutively share one upload).  Everything else as
        zoom_fovs; with both None the call is gfw_zoom_fovs's."""
        n = len(frames)
        arr = frames if isinstance(frames, C.Array) else (abi.ZoomFrame * max(n, 1))(*frames)
        rp = None
        if rotations is not None:
            rot = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1, 9)
            assert rot.shape[0] == n
            rp = rot.ctypes.data
        sp, _keep = (None, None)
        if stabs is not None:
            assert len(stabs) == n
            sp, _keep = frame_stab_table(stabs)
        mp = lp = None
        if meshes is not None:
            assert len(meshes) == n
            mp, lp, _held = frame_mesh_table(meshes)
        if out_ptr is not None:
            self._check(self.lib.gfw_zoom_fovs_stab(self.ctx, C.byref(params), C.byref(search), C.cast(arr, C.c_void_p), n, rp, sp, mp, lp, out_ptr, debug_ptr, 1))
            return None
        fov = np.zeros(n, dtype=np.float64)
        dbg = np.zeros((n, abi.ZOOM_RECT_POINTS, 2), dtype=np.float64) if debug else None
        self._check(self.lib.gfw_zoom_fovs_stab(self.ctx, C.byref(params), C.byref(search), C.cast(arr, C.c_void_p), n, rp, sp, mp, lp, fov.ctypes.data,
                                                dbg.ctypes.data if debug else None, 0))
        return (fov, dbg) if debug else fov

    @staticmethod
    def _sync_pairs(pairs):
        """[(ts_us, next_ts_us, points_a [n][2], points_b [n][2])] -> the flat arrays gfw_sync_visual_* take (kept alive by the caller)"""
        ts = np.array([[int(a), int(b)] for a, b, _, _ in pairs], dtype=np.int64).reshape(-1, 2)
        pa = [np.asarray(x, dtype=np.float32).reshape(-1, 2) for _, _, x, _ in pairs]
        pb = [np.asarray(x, dtype=np.float32).reshape(-1, 2) for _, _, _, x in pairs]
        assert all(a.shape == b.shape for a, b in zip(pa, pb)), "a pair's two point sets have one length"
        first = np.zeros(len(pairs) + 1, dtype=np.int32)
        if pairs:
            first[1:] = np.cumsum([len(a) for a in pa])
        cat = lambda v: np.ascontiguousarray(np.concatenate(v), dtype=np.float32) if v else np.zeros((0, 2), dtype=np.float32)
        return ts, first, cat(pa), cat(pb)

    def sync_visual_costs(self, params, search, pairs, candidates, mapped=False, out_ptr=None, mapped_ptr=None):
        """calculate_distance (find_offset/visual_features.rs:49-83) of every candidate in one device call (gfw_sync_visual_costs).

        ``params``: the KernelParams `undistort_points` builds; ``search``: abi.SyncSearch; ``pairs``: [(ts_us, next_ts_us, points [n][2], points [n][2])];
        ``candidates``: [n][2] (offset_ms, frame_readout_time_ms).  Returns float64 [n] — with ``mapped`` also float32 [n][total][2][2], p1 and p2 as
        mapped — or, with ``out_ptr`` (a device pointer to n doubles; ``mapped_ptr``: None or a device pointer), None: in order on the stream."""
        ts, first, pa, pb = self._sync_pairs(pairs)
        cand = np.ascontiguousarray(candidates, dtype=np.float64).reshape(-1, 2)
        n, total = cand.shape[0], int(first[-1])
        args = (self.ctx, C.byref(params), C.byref(search), ts.ctypes.data, first.ctypes.data, pa.ctypes.data, pb.ctypes.data, len(pairs), cand.ctypes.data, n)
        if out_ptr is not None:
            self._check(self.lib.gfw_sync_visual_costs(*args, out_ptr, mapped_ptr, 1))
            return None
        costs = np.zeros(n, dtype=np.float64)
        pts = np.zeros((n, total, 2, 2), dtype=np.float32) if mapped else None
        self._check(self.lib.gfw_sync_visual_costs(*args, costs.ctypes.data, pts.ctypes.data if mapped else None, 0))
        return (costs, pts) if mapped else costs

    def sync_visual_search(self, params, search, pairs, mode, initial_offset_ms=0.0, search_size_ms=0.0, frame_readout_time_ms=0.0, scaled_fps=30.0,
                           costs=False, result_ptr=None, coarse_ptr=None, fine_ptr=None):
        """The two-stage search of one range (visual_features.rs:87-131) in one device call (gfw_sync_visual_search): ``mode`` 0 the offset, 1 the readout time.
        Returns abi.SyncResult — with ``costs`` also the coarse [n_coarse] and fine [200] float64 costs — or, with ``result_ptr`` (a device pointer to a
        gfw_sync_result; ``coarse_ptr`` / ``fine_ptr``: None or device pointers), None: in order on the stream."""
        ts, first, pa, pb = self._sync_pairs(pairs)
        args = (self.ctx, C.byref(params), C.byref(search), ts.ctypes.data, first.ctypes.data, pa.ctypes.data, pb.ctypes.data, len(pairs), int(mode),
                float(initial_offset_ms), float(search_size_ms), float(frame_readout_time_ms), float(scaled_fps))
        if result_ptr is not None:
            self._check(self.lib.gfw_sync_visual_search(*args, result_ptr, coarse_ptr, fine_ptr, 1))
            return None
        res = abi.SyncResult()
        n_coarse = sync_coarse_count(mode, search_size_ms, scaled_fps)
        coarse, fine = np.zeros(max(n_coarse, 1), dtype=np.float64), np.zeros(abi.SYNC_FINE_CANDIDATES, dtype=np.float64)
        self._check(self.lib.gfw_sync_visual_search(*args, C.cast(C.byref(res), C.c_void_p), coarse.ctypes.data if costs else None, fine.ctypes.data if costs else None, 0))
        return (res, coarse[:n_coarse], fine) if costs else res

    @staticmethod
    def _sync_gyro_ranges(ranges):
        """[(est [n][4], est_has [n] or None, gyro [m][4], gyro_has [m] or None)] — rows (timestamp_ms, x, y, z) — -> the flat arrays gfw_sync_gyro_* take (kept alive by the caller)"""
        def flat(col_data, col_has):
            data = [np.asarray(r[col_data], dtype=np.float64).reshape(-1, 4) for r in ranges]
            has = [np.ones(len(d), dtype=np.uint8) if r[col_has] is None else (np.asarray(r[col_has]).reshape(-1) != 0).astype(np.uint8) for r, d in zip(ranges, data)]
            assert all(len(d) == len(h) for d, h in zip(data, has)), "one has byte per sample"
            first = np.zeros(len(ranges) + 1, dtype=np.int32)
            if ranges:
                first[1:] = np.cumsum([len(d) for d in data])
            cat = np.ascontiguousarray(np.concatenate(data)) if data else np.zeros((0, 4))
            return first, cat, (np.ascontiguousarray(np.concatenate(has)) if has else np.zeros(0, dtype=np.uint8))
        return flat(0, 1) + flat(2, 3)

    def sync_gyro_costs(self, ranges, candidates, out_ptr=None):
        """calculate_cost (find_offset/essential_matrix.rs:109-131) of caller-given candidate offsets for every range in one device call (gfw_sync_gyro_costs).

        ``ranges``: [(est [n][4], est_has or None, gyro [m][4], gyro_has or None)], rows (timestamp_ms, x, y, z), the gyro slice cut to the range's window and
        filtered; ``candidates``: one float64 array of offsets (ms) per range.  Returns one float64 cost array per range — or, with ``out_ptr`` (a device
        pointer to as many doubles as there are candidates, range after range), None: in order on the stream."""
        ef, e, eh, gf, g, gh = self._sync_gyro_ranges(ranges)
        cands = [np.asarray(c, dtype=np.float64).reshape(-1) for c in candidates]
        assert len(cands) == len(ranges)
        cf = np.zeros(len(ranges) + 1, dtype=np.int32)
        if cands:
            cf[1:] = np.cumsum([len(c) for c in cands])
        cand = np.ascontiguousarray(np.concatenate(cands)) if cands else np.zeros(0)
        args = (self.ctx, ef.ctypes.data, e.ctypes.data, eh.ctypes.data, len(e), gf.ctypes.data, g.ctypes.data, gh.ctypes.data, len(g), len(ranges),
                cf.ctypes.data, cand.ctypes.data, len(cand))
        if out_ptr is not None:
            self._check(self.lib.gfw_sync_gyro_costs(*args, out_ptr, 1))
            return None
        costs = np.zeros(max(len(cand), 1), dtype=np.float64)
        self._check(self.lib.gfw_sync_gyro_costs(*args, costs.ctypes.data, 0))
        return [costs[cf[r]:cf[r + 1]].copy() for r in range(len(ranges))]

    def sync_gyro_search(self, ranges, initial_offset_ms=0.0, search_size_ms=5000.0, costs=False, result_ptr=None, coarse_ptr=None, fine_ptr=None):
        """The two-stage search of essential_matrix.rs:52-75 for every range in one device call (gfw_sync_gyro_search); ``ranges`` as for sync_gyro_costs.
        Returns [abi.SyncResult] — with ``costs`` also the coarse [n_ranges][n_coarse] and fine [n_ranges][200] float64 costs — or, with ``result_ptr`` (a
        device pointer to n_ranges gfw_sync_result; ``coarse_ptr`` / ``fine_ptr``: None or device pointers), None: in order on the stream."""
        ef, e, eh, gf, g, gh = self._sync_gyro_ranges(ranges)
        n = len(ranges)
        args = (self.ctx, ef.ctypes.data, e.ctypes.data, eh.ctypes.data, len(e), gf.ctypes.data, g.ctypes.data, gh.ctypes.data, len(g), n,
                float(initial_offset_ms), float(search_size_ms))
        if result_ptr is not None:
            self._check(self.lib.gfw_sync_gyro_search(*args, result_ptr, coarse_ptr, fine_ptr, 1))
            return None
        res = (abi.SyncResult * max(n, 1))()
        n_coarse = sync_gyro_coarse_count(search_size_ms)
        coarse, fine = np.zeros(max(n * n_coarse, 1), dtype=np.float64), np.zeros((max(n, 1), abi.SYNC_FINE_CANDIDATES), dtype=np.float64)
        self._check(self.lib.gfw_sync_gyro_search(*args, C.cast(res, C.c_void_p), coarse.ctypes.data if costs else None, fine.ctypes.data if costs else None, 0))
        out = [res[i] for i in range(n)]
        return (out, coarse[:n * n_coarse].reshape(n, n_coarse), fine[:n]) if costs else out

    def sync_optim_rank(self, gyro, sample_rate, out_ptrs=None):
        """The band energies and the rank of every window of a gyro series (optimsync.rs:73-149) in one device call (gfw_sync_optim_rank).
        ``gyro``: [3][S] float64, axis after axis (``optim_resample``).  Returns (lf, mf, hf, rank) float32 [n_windows] — or, with ``out_ptrs`` (four device
        pointers or None each, to n_windows floats), the window count: in order on the stream."""
        g = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1))
        s = g.shape[1]
        n_w = C.c_int32(0)
        args = (self.ctx, g.ctypes.data if s else None, s, float(sample_rate))
        if out_ptrs is not None:
            self._check(self.lib.gfw_sync_optim_rank(*args, *out_ptrs, C.addressof(n_w), 1))
            return n_w.value
        cap = max(s // 16 + 1, 1)
        outs = [np.zeros(cap, dtype=np.float32) for _ in range(4)]
        self._check(self.lib.gfw_sync_optim_rank(*args, *[o.ctypes.data for o in outs], C.addressof(n_w), 0))
        return tuple(o[:n_w.value] for o in outs)

    def sync_optim_points(self, gyro, sample_rate, target_sync_points, trim_ranges_s, details=False, out_ptrs=None):
        """OptimSync::run (optimsync.rs:68-225) in one device call (gfw_sync_optim_points): where in the clip to sync.  ``trim_ranges_s``: [(from_s, to_s)].
        Returns (points_ms float64, rank float32 [n_windows] before the masks, ratio) — with ``details`` also rank_nms — or, with ``out_ptrs`` = (points_ms,
        n_points, rank or None, rank_nms or None) device pointers, the ratio: in order on the stream."""
        g = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64).reshape(3, -1))
        s = g.shape[1]
        tr = np.ascontiguousarray(np.asarray(list(trim_ranges_s), dtype=np.float64).reshape(-1, 2))
        ratio = C.c_double(0.0)
        args = (self.ctx, g.ctypes.data if s else None, s, float(sample_rate), int(target_sync_points), tr.ctypes.data if len(tr) else None, len(tr))
        if out_ptrs is not None:
            self._check(self.lib.gfw_sync_optim_points(*args, *out_ptrs, C.addressof(ratio), 1))
            return ratio.value
        cap = max(s // 16 + 1, 1)
        pts, n_pts = np.zeros(max(int(target_sync_points), 1), dtype=np.float64), C.c_int32(0)
        rank, nms = np.zeros(cap, dtype=np.float32), np.zeros(cap, dtype=np.float32)
        self._check(self.lib.gfw_sync_optim_points(*args, pts.ctypes.data, C.addressof(n_pts), rank.ctypes.data, nms.ctypes.data if details else None, C.addressof(ratio), 0))
        n_w = optim_window_count(s, sample_rate)
        out = (pts[:n_pts.value], rank[:n_w], ratio.value)
        return out + (nms[:n_w],) if details else out

    @staticmethod
    def _pose_pairs(pairs):
        """[(points_a [n][2], points_b [n][2])] -> (pair_first, points_a, points_b) as gfw_pose_almeida takes them (kept alive by the caller)"""
        _, first, pa, pb = Backend._sync_pairs([(0, 0, a, b) for a, b in pairs])
        return first, pa, pb

    def pose_almeida(self, params, cfg, pairs, triples, samples=None, rounds=False, out_ptrs=None):
        """PoseAlmeida::estimate_pose (estimate_pose/almeida.rs:23-238) of every frame pair in one device call (gfw_pose_almeida), the random draws given.

        ``params``: the KernelParams `undistort_points` builds; ``cfg``: abi.PoseAlmeidaCfg; ``pairs``: [(points_a [n][2], points_b [n][2])] optical-flow pixels;
        ``triples``: int32 [n_pairs][num_iters][3]; ``samples``: None (every round's list is 0 .. n-1) or one int32 array [num_iters][min(n, num_samples)] per pair
        (``pose_draws`` makes both).  Returns (quats f32 [n_pairs][4] (w, i, j, k), rotations f64 [n_pairs][3][3], best int32 [n_pairs][2] (inliers, round)) — with
        ``rounds`` also every round's inliers int32 [n_pairs][num_iters] and fit f32 [n_pairs][num_iters][4] — or, with ``out_ptrs`` = (quats, rotations, best,
        round_inliers or None, round_fits or None) device pointers, None: in order on the stream."""
        first, pa, pb = self._pose_pairs(pairs)
        n, iters = len(pairs), int(cfg.num_iters)
        tr = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1)
        assert tr.size == n * iters * 3, "triples: [n_pairs][num_iters][3]"
        sf = sm = None
        if samples is not None:
            lists = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in samples]
            assert len(lists) == n
            sf = np.zeros(n + 1, dtype=np.int32)
            if n:
                sf[1:] = np.cumsum([len(s) for s in lists])
            sm = np.ascontiguousarray(np.concatenate(lists)) if lists else np.zeros(0, dtype=np.int32)
            if not sm.size:
                sm = np.zeros(1, dtype=np.int32)
        p = lambda a: a.ctypes.data if a is not None else None
        args = (self.ctx, C.byref(params), C.byref(cfg), first.ctypes.data, pa.ctypes.data, pb.ctypes.data, n, tr.ctypes.data if tr.size else None, p(sf), p(sm))
        if out_ptrs is not None:
            self._check(self.lib.gfw_pose_almeida(*args, *out_ptrs, 1))
            return None
        quats, rot, best = np.zeros((n, 4), dtype=np.float32), np.zeros((n, 3, 3), dtype=np.float64), np.zeros((n, 2), dtype=np.int32)
        ri, rf = np.zeros((n, iters), dtype=np.int32), np.zeros((n, iters, 4), dtype=np.float32)
        q = lambda a: a.ctypes.data if a.size else None
        self._check(self.lib.gfw_pose_almeida(*args, q(quats), q(rot), q(best), q(ri) if rounds else None, q(rf) if rounds else None, 0))
        return (quats, rot, best, ri, rf) if rounds else (quats, rot, best)

    def pose_essential(self, params, cfg, pairs, octets, rounds=False, out_ptrs=None):
        """Essential-matrix pose estimation (pose methods 0 and 2 of estimate_pose/mod.rs:27-36) of every frame pair in one device call (gfw_pose_essential), the
        random draws given: the rotation part of an essential matrix fitted to the pair's undistorted bearings.  Neither OpenCV's LMedS nor ARRSAC is reproduced.

        ``params``: the KernelParams `undistort_points` builds; ``cfg``: abi.PoseEssentialCfg; ``pairs``: [(points_a [n][2], points_b [n][2])] optical-flow pixels;
        ``octets``: int32 [n_pairs][num_iters][8] (``pose_draws_k`` makes them).  Returns (quats f32 [n_pairs][4] (w, i, j, k), rotations f64 [n_pairs][3][3],
        essential f64 [n_pairs][9], best int32 [n_pairs][4] (inliers, round, front, found)) — with ``rounds`` also every round's inliers int32 [n_pairs][num_iters]
        and fit f64 [n_pairs][num_iters][9] — or, with ``out_ptrs`` = (quats, rotations, essential, best, round_inliers or None, round_fits or None) device
        pointers, None: in order on the stream."""
        first, pa, pb = self._pose_pairs(pairs)
        n, iters = len(pairs), int(cfg.num_iters)
        oc = np.ascontiguousarray(octets, dtype=np.int32).reshape(-1)
        assert oc.size == n * iters * 8, "octets: [n_pairs][num_iters][8]"
        args = (self.ctx, C.byref(params), C.byref(cfg), first.ctypes.data, pa.ctypes.data, pb.ctypes.data, n, oc.ctypes.data if oc.size else None)
        if out_ptrs is not None:
            self._check(self.lib.gfw_pose_essential(*args, *out_ptrs, 1))
            return None
        quats, rot, ess, best = np.zeros((n, 4), dtype=np.float32), np.zeros((n, 3, 3)), np.zeros((n, 9)), np.zeros((n, 4), dtype=np.int32)
        ri, rf = np.zeros((n, iters), dtype=np.int32), np.zeros((n, iters, 9))
        q = lambda a: a.ctypes.data if a.size else None
        self._check(self.lib.gfw_pose_essential(*args, q(quats), q(rot), q(ess), q(best), q(ri) if rounds else None, q(rf) if rounds else None, 0))
        return (quats, rot, ess, best, ri, rf) if rounds else (quats, rot, ess, best)

    @staticmethod
    def _sync_rs_ranges(ranges):
        """[[(ts_a_us, ts_b_us, points_a [n][2], points_b [n][2])]] -> (range_first, pair_ts, pair_first, points_a, points_b) as gfw_sync_rs_* take them"""
        rf = np.zeros(len(ranges) + 1, dtype=np.int32)
        if ranges:
            rf[1:] = np.cumsum([len(r) for r in ranges])
        ts, first, pa, pb = Backend._sync_pairs([p for r in ranges for p in r])
        return rf, ts, first, pa, pb

    def sync_rs_costs(self, params, cfg, ranges, track_ts_us, track_wxyz, candidates, out_ptr=None):
        """The rs-sync range costs (find_offset/rs_sync.rs; the solver as tests/_rssyncstmt.py states it) of caller-given candidate delays for every range in one
        device call (gfw_sync_rs_costs).

        ``params``: the KernelParams `undistort_points` builds; ``cfg``: abi.SyncRsCfg; ``ranges``: one list of (ts_a_us, ts_b_us, points_a [n][2], points_b
        [n][2]) optical-flow pairs per range; ``track_ts_us`` int64 [n] strictly ascending, ``track_wxyz`` f64 [n][4]: the quaternion track; ``candidates``: one
        float64 array of delays (seconds) per range.  Returns one float64 cost array per range — or, with ``out_ptr`` (a device pointer to as many doubles as
        there are candidates, range after range), None: in order on the stream."""
        rf, ts, first, pa, pb = self._sync_rs_ranges(ranges)
        tt, tq = np.ascontiguousarray(track_ts_us, dtype=np.int64).reshape(-1), np.ascontiguousarray(track_wxyz, dtype=np.float64).reshape(-1, 4)
        assert len(tt) == len(tq), "one quaternion per track timestamp"
        cands = [np.asarray(c, dtype=np.float64).reshape(-1) for c in candidates]
        assert len(cands) == len(ranges)
        cf = np.zeros(len(ranges) + 1, dtype=np.int32)
        if cands:
            cf[1:] = np.cumsum([len(c) for c in cands])
        cand = np.ascontiguousarray(np.concatenate(cands)) if cands else np.zeros(0)
        args = (self.ctx, C.byref(params), C.byref(cfg), rf.ctypes.data, len(ranges), ts.ctypes.data, first.ctypes.data, pa.ctypes.data, pb.ctypes.data, len(ts),
                tt.ctypes.data, tq.ctypes.data, len(tt), cf.ctypes.data, cand.ctypes.data, len(cand))
        if out_ptr is not None:
            self._check(self.lib.gfw_sync_rs_costs(*args, out_ptr, 1))
            return None
        costs = np.zeros(max(len(cand), 1), dtype=np.float64)
        self._check(self.lib.gfw_sync_rs_costs(*args, costs.ctypes.data, 0))
        return [costs[cf[r]:cf[r + 1]].copy() for r in range(len(ranges))]

    def sync_rs_search(self, params, cfg, ranges, track_ts_us, track_wxyz, initial_delay_s=0.0, radius_s=3.0, rounds=False, out_ptrs=None):
        """``full_sync`` of rs_sync.rs:164-175 for every range in one device call (gfw_sync_rs_search); arguments as for sync_rs_costs, delays in seconds.
        Returns [abi.SyncResult] (coarse_value / coarse_cost: the round-0 pick; value / cost: the final delay and its pick's cost) — with ``rounds`` also every
        round's candidates and range costs, f64 [n_ranges][sync_rs_candidates(..)] each — or, with ``out_ptrs`` = (results, round_candidates or None,
        round_costs or None) device pointers, None: in order on the stream."""
        rf, ts, first, pa, pb = self._sync_rs_ranges(ranges)
        tt, tq = np.ascontiguousarray(track_ts_us, dtype=np.int64).reshape(-1), np.ascontiguousarray(track_wxyz, dtype=np.float64).reshape(-1, 4)
        assert len(tt) == len(tq), "one quaternion per track timestamp"
        n = len(ranges)
        args = (self.ctx, C.byref(params), C.byref(cfg), rf.ctypes.data, n, ts.ctypes.data, first.ctypes.data, pa.ctypes.data, pb.ctypes.data, len(ts),
                tt.ctypes.data, tq.ctypes.data, len(tt), float(initial_delay_s), float(radius_s))
        if out_ptrs is not None:
            self._check(self.lib.gfw_sync_rs_search(*args, *out_ptrs, 1))
            return None
        res = (abi.SyncResult * max(n, 1))()
        total = sync_rs_candidates(radius_s, cfg.step_s, cfg.rounds) if rounds else 0
        cand, cost = np.zeros((n, total)), np.zeros((n, total))
        q = lambda a: a.ctypes.data if a.size else None
        self._check(self.lib.gfw_sync_rs_search(*args, C.cast(res, C.c_void_p), q(cand) if rounds else None, q(cost) if rounds else None, 0))
        out = [res[i] for i in range(n)]
        return (out, cand, cost) if rounds else out

    @staticmethod
    def _flow_features(features):
        """one [n][2] array per frame -> (feat_first int32 [n_frames + 1], features f32 [total][2]) as gfw_flow_pyrlk takes them (kept alive by the caller)"""
        lists = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 2) for f in features]
        first = np.zeros(len(lists) + 1, dtype=np.int32)
        if lists:
            first[1:] = np.cumsum([len(f) for f in lists])
        pts = np.ascontiguousarray(np.concatenate(lists)) if lists else np.zeros((0, 2), dtype=np.float32)
        return first, (pts if pts.size else np.zeros((1, 2), dtype=np.float32))

    def flow_pyrlk(self, frames, width, pairs, features=None, iters=False, out_ptrs=None, shape=None, point_mode=None):
        """`OFOpenCVPyrLK::optical_flow_to` (optical_flow/opencv_pyrlk.rs:63-119) of every frame pair in one device call (gfw_flow_pyrlk): pyramidal Lucas-Kanade
        tracking of each pair's first-frame features into its second frame, and the filter of the result.

        ``frames``: u8 gray planes as numpy [n][height][stride], or a device pointer (int) with ``shape`` = (n, height, stride); ``width`` <= stride; ``pairs``:
        [(first frame, second frame)]; ``features``: one f32 [..][2] array per frame (pixels), or None for the grid points of opencv_dis.rs:62-119 computed on the
        device.  Returns a dict: next f32 [raw][2], status u8 [raw], pair_first int32 [n_pairs + 1], points_a / points_b f32 [kept][2] (what pose_almeida and the
        visual search take) — with ``iters`` also iters int32 [raw][4], in the grid mode also grid_points f32 [n][nodes][2] and grid_counts int32 [n] — or, with
        ``out_ptrs`` = (next, status, iters or None, grid_points or None, grid_counts or None, pair_first, points_a, points_b) device pointers (points_a / points_b
        with room for [raw][2]), the number of raw slots: in order on the stream."""
        fp, on_device, (n, height, stride), _keep = _frames_arg(frames, shape)
        mode = (1 if features is None else 0) if point_mode is None else int(point_mode)
        cfg = abi.FlowPyrLKCfg(width=int(width), height=int(height), stride=int(stride), point_mode=mode)
        pf = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        ff, ft = (None, None) if features is None else self._flow_features(features)
        p = lambda a: a.ctypes.data if a is not None and a.size else None
        args = (self.ctx, C.byref(cfg), fp, on_device, int(n), p(pf), len(pf), p(ff), p(ft))
        raw = flow_raw_slots(width, height, pf, ff if mode == 0 else None) if (mode == 1 or ff is not None) else 0
        if out_ptrs is not None:
            self._check(self.lib.gfw_flow_pyrlk(*args, *out_ptrs, 1))
            return raw
        grid = mode == 1
        nodes = flow_grid_nodes(width, height) if grid and width >= 15 else 0
        room = max(raw, 1)                                       # (an output without slots still is an array of the caller's: at least one element)
        o = {"next": np.zeros((room, 2), dtype=np.float32), "status": np.zeros(room, dtype=np.uint8), "iters": np.zeros((room, 4), dtype=np.int32),
             "pair_first": np.zeros(len(pf) + 1, dtype=np.int32), "points_a": np.zeros((room, 2), dtype=np.float32), "points_b": np.zeros((room, 2), dtype=np.float32),
             "grid_points": np.zeros((n, nodes, 2), dtype=np.float32), "grid_counts": np.zeros(n, dtype=np.int32)}
        self._check(self.lib.gfw_flow_pyrlk(*args, o["next"].ctypes.data, o["status"].ctypes.data, o["iters"].ctypes.data if iters else None, p(o["grid_points"]) if grid else None,
                                            p(o["grid_counts"]) if grid else None, o["pair_first"].ctypes.data, o["points_a"].ctypes.data, o["points_b"].ctypes.data, 0))
        kept = int(o["pair_first"][-1]) if len(pf) else 0
        o["next"], o["status"], o["iters"] = o["next"][:raw], o["status"][:raw], o["iters"][:raw]
        o["points_a"], o["points_b"] = o["points_a"][:kept], o["points_b"][:kept]
        if not iters:
            del o["iters"]
        if not grid:
            del o["grid_points"], o["grid_counts"]
        return o

    def flow_dis(self, frames, width, pairs, finest_scale=2, flow=False, out_ptrs=None, shape=None, variational_iters=0, varref=None):
        """`OFOpenCVDis` (optical_flow/opencv_dis.rs, the reference's default method 2) of every frame pair in one device call (gfw_flow_dis): the DIS dense flow
        with the parameters of DISOpticalFlow_PRESET_FAST, read at the grid points of opencv_dis.rs:62-119.  ``variational_iters`` = 0 (the default) is the flow
        WITHOUT the preset's variational refinement; n > 0 goes to gfw_flow_dis_refined with n fixed-point iterations on every level (the preset: 5) and the
        other parameters of ``varref`` (an ``abi.FlowVarrefCfg``; None: ``abi.varref_cfg()``, the preset's values to the builder's best knowledge).

        ``frames``: u8 gray planes as numpy [n][height][stride], or a device pointer (int) with ``shape`` = (n, height, stride); ``width`` <= stride; ``pairs``:
        [(first frame, second frame)]; ``finest_scale`` 2 (the reference's) or 1.  Returns a dict: grid_points f32 [n][nodes][2], grid_counts int32 [n], pair_first
        int32 [n_pairs + 1], points_a / points_b f32 [total][2] (every kept node of each pair's first frame and where the flow takes it: what pose_almeida and the
        visual search take) — with ``flow`` also flow f32 [n_pairs][height >> finest_scale][width >> finest_scale][2], the finest level's dense field — or, with
        ``out_ptrs`` = (grid_points or None, grid_counts or None, flow or None, pair_first, points_a, points_b) device pointers (points_a / points_b with room for
        [n_pairs * nodes][2]), the number of those slots: in order on the stream."""
        fp, on_device, (n, height, stride), _keep = _frames_arg(frames, shape)
        cfg = abi.FlowDisCfg(width=int(width), height=int(height), stride=int(stride), finest_scale=int(finest_scale))
        pf = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        p = lambda a: a.ctypes.data if a is not None and a.size else None
        if int(variational_iters) == 0 and varref is None:
            call, args = self.lib.gfw_flow_dis, (self.ctx, C.byref(cfg), fp, on_device, int(n), p(pf), len(pf))
        else:
            ref = abi.varref_cfg() if varref is None else abi.FlowVarrefCfg.from_buffer_copy(varref)
            ref.fixed_point_iters = int(variational_iters)
            call, args = self.lib.gfw_flow_dis_refined, (self.ctx, C.byref(cfg), C.byref(ref), fp, on_device, int(n), p(pf), len(pf))
        nodes = flow_grid_nodes(width, height) if width >= 15 else 0
        if out_ptrs is not None:
            self._check(call(*args, *out_ptrs, 1))
            return len(pf) * nodes
        room = max(len(pf) * nodes, 1)                           # (an output without slots still is an array of the caller's: at least one element)
        fs = int(finest_scale) if int(finest_scale) in (1, 2) else 2
        o = {"grid_points": np.zeros((n, nodes, 2), dtype=np.float32), "grid_counts": np.zeros(n, dtype=np.int32),
             "flow": np.zeros((len(pf) if flow else 0, int(height) >> fs, int(width) >> fs, 2), dtype=np.float32),
             "pair_first": np.zeros(len(pf) + 1, dtype=np.int32), "points_a": np.zeros((room, 2), dtype=np.float32), "points_b": np.zeros((room, 2), dtype=np.float32)}
        self._check(call(*args, p(o["grid_points"]), p(o["grid_counts"]), p(o["flow"]) if flow else None, o["pair_first"].ctypes.data,
                    o["points_a"].ctypes.data, o["points_b"].ctypes.data, 0))
        total = int(o["pair_first"][-1]) if len(pf) else 0
        o["points_a"], o["points_b"] = o["points_a"][:total], o["points_b"][:total]
        if not flow:
            del o["flow"]
        return o

    def corners_shi_tomasi(self, frames, width, max_corners=200, quality=0.01, min_distance=10.0, scores=False, packed=True, max_workspace_mb=0, out_ptrs=None, shape=None):
        """`OFOpenCVPyrLK::detect_features` (optical_flow/opencv_pyrlk.rs:25-42: good_features_to_track(img, 200, 0.01, 10.0, ..)) of every frame in one device call
        (gfw_corners_shi_tomasi): Shi-Tomasi corners by the minimum eigenvalue of the 3 x 3 gradient covariance, thresholded at ``quality`` of the frame's maximum,
        picked in descending order at least ``min_distance`` apart.

        ``frames``: u8 gray planes as numpy [n][height][stride], or a device pointer (int) with ``shape`` = (n, height, stride); ``width`` <= stride.  Returns a dict:
        corners f32 [n][max_corners][2] (kept first, in pick order, then zeros), counts int32 [n] — with ``scores`` also scores f32 [n][max_corners], with ``packed``
        also feat_first int32 [n + 1] and features f32 [kept][2], what flow_pyrlk takes as its features — or, with ``out_ptrs`` = (corners, scores or None, counts,
        feat_first or None, features or None) device pointers (features with room for [n * max_corners][2]), None: in order on the stream."""
        fp, on_device, (n, height, stride), _keep = _frames_arg(frames, shape)
        cfg = abi.CornersCfg(width=int(width), height=int(height), stride=int(stride), max_corners=int(max_corners), quality=float(quality), min_distance=float(min_distance),
                             max_workspace_mb=int(max_workspace_mb))
        args = (self.ctx, C.byref(cfg), fp, on_device, int(n))
        if out_ptrs is not None:
            self._check(self.lib.gfw_corners_shi_tomasi(*args, *out_ptrs, 1))
            return None
        room = max(int(n) * max(int(max_corners), 0), 1)             # (an output without slots still is an array of the caller's: at least one element)
        o = {"corners": np.zeros((room, 2), dtype=np.float32), "scores": np.zeros(room, dtype=np.float32), "counts": np.zeros(max(n, 1), dtype=np.int32),
             "feat_first": np.zeros(n + 1, dtype=np.int32), "features": np.zeros((room, 2), dtype=np.float32)}
        self._check(self.lib.gfw_corners_shi_tomasi(*args, o["corners"].ctypes.data, o["scores"].ctypes.data if scores else None, o["counts"].ctypes.data,
                                                    o["feat_first"].ctypes.data if packed else None, o["features"].ctypes.data if packed else None, 0))
        m = max(int(max_corners), 0)
        o["corners"], o["scores"], o["counts"] = o["corners"][:n * m].reshape(n, m, 2), o["scores"][:n * m].reshape(n, m), o["counts"][:n]
        o["features"] = o["features"][:int(o["feat_first"][-1])]
        if not scores:
            del o["scores"]
        if not packed:
            del o["feat_first"], o["features"]
        return o

    def synchronize(self):
        self._check(self.lib.gfw_synchronize(self.ctx))

    def flush(self):
        """Enqueue whatever plane coalescing holds for a frame this context belongs to (gfw_flush); does not wait for the GPU."""
        self._check(self.lib.gfw_flush(self.ctx))

    def undistort_image(self, buffers, params, matrices, mesh=None, matrix_count=None):
        """One plane (OclWrapper::undistort_image).  ``matrices``: numpy [rows][14] f32, or a device pointer int."""
        mp, mc, _m = _matrix_arg(matrices, matrix_count)
        meshp, meshn, _mesh = _mesh_arg(mesh)
        self._check(self.lib.gfw_undistort_image(self.ctx, C.byref(buffers), C.byref(params), mp, mc, None, 0, meshp, meshn))

    def undistort_frame(self, planes, params, pixel_types, matrices, mesh=None, matrix_count=None):
        """All planes of a frame in one call (additive entry point)."""
        n = len(planes)
        barr = (abi.Buffers * n)(*planes)
        parr = (abi.KernelParams * n)(*params)
        tarr = (C.c_int * n)(*[abi.PIXEL_TYPES[t][0] if isinstance(t, str) else t for t in pixel_types])
        mp, mc, _m = _matrix_arg(matrices, matrix_count)
        meshp, meshn, _mesh = _mesh_arg(mesh)
        self._check(self.lib.gfw_undistort_frame(self.ctx, n, barr, parr, tarr, mp, mc, meshp, meshn))


def flow_grid_nodes(width, height):
    """raw slots of a pair in gfw_flow_pyrlk's grid mode: the nodes of `(0..w).step_by(w / 15)` x `(0..h).step_by(w / 15)` (opencv_dis.rs:64, :109-110)"""
    step = int(width) // 15
    return ((int(width) + step - 1) // step) * ((int(height) + step - 1) // step)


def flow_raw_slots(width, height, pair_frames, feat_first=None):
    """raw slots of a gfw_flow_pyrlk call: every pair's first-frame features (``feat_first`` [n_frames + 1]), or with None every node of the grid per pair"""
    pf = np.asarray(pair_frames).reshape(-1, 2)
    if feat_first is None:
        return len(pf) * flow_grid_nodes(width, height)
    return int(sum(int(feat_first[a + 1]) - int(feat_first[a]) for a in pf[:, 0] if 0 <= a < len(feat_first) - 1))


def sync_coarse_count(mode, search_size_ms, scaled_fps):
    """candidates of the first stage: `search_size as usize` (visual_features.rs:113), or `-steps..steps` with steps = (1000.0 / fps) as isize (:89-91)"""
    v = float(search_size_ms) if int(mode) == 0 else (1000.0 / float(scaled_fps) if scaled_fps else float("inf"))
    steps = 0 if v != v or v <= 0.0 else int(min(v, 2.0 ** 62))
    return steps if int(mode) == 0 else 2 * steps


def sync_gyro_coarse_count(search_size_ms):
    """candidates of the gyro-match search's first stage: `search_size as usize * 2` (essential_matrix.rs:55) — the cast comes before the multiplication"""
    v = float(search_size_ms)
    return 0 if v != v or v <= 0.0 else int(min(v, 2.0 ** 62)) * 2


def sync_rs_candidates(radius_s, step_s, rounds):
    """candidates of a range over all rounds of gfw_sync_rs_search: 2 floor(radius / step) + 1, then 17 a round"""
    return 2 * int(np.floor(float(radius_s) / float(step_s))) + 1 + (int(rounds) - 1) * abi.SYNC_RS_LATER


def optim_window_count(n_samples, sample_rate):
    """windows of gfw_sync_optim_*: `windows(fft_size).step_by(16)` with fft_size = `sample_rate.round() as usize` (optimsync.rs:82, :93-94)"""
    v = float(sample_rate)
    n = 0 if v != v or v <= 0.0 else int(min(np.floor(v + 0.5), 2.0 ** 62))
    return 0 if n < 1 or n_samples < n else (int(n_samples) - n) // 16 + 1


def optim_resample(timestamps_ms, xyz, has=None):
    """OptimSync::new (optimsync.rs:30-66) on the host (gfw_optim_resample; no context, no GPU): the gyro resampled at its average rate -> (float64 [3][S], sample_rate).
    ``has``: None or [n], 0 = `gyro: None`."""
    ts = np.ascontiguousarray(np.asarray(timestamps_ms, dtype=np.float64).reshape(-1))
    v = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    h = None if has is None else np.ascontiguousarray((np.asarray(has).reshape(-1) != 0).astype(np.uint8))
    assert len(v) == len(ts) and (h is None or len(h) == len(ts))
    lib = abi.load_library()
    n_out, rate = C.c_int64(0), C.c_double(0.0)
    args = (ts.ctypes.data if len(ts) else None, v.ctypes.data if len(ts) else None, h.ctypes.data if h is not None and len(h) else None, len(ts))
    rc = lib.gfw_optim_resample(*args, None, 0, C.addressof(n_out), C.addressof(rate))
    if rc < 0:
        raise GfwError(rc, lib.gfw_last_error().decode())
    out = np.zeros((3, n_out.value), dtype=np.float64)
    if out.size:
        rc = lib.gfw_optim_resample(*args, out.ctypes.data, n_out.value, C.addressof(n_out), C.addressof(rate))
        if rc < 0:
            raise GfwError(rc, lib.gfw_last_error().decode())
    return out, rate.value


def pose_draws(seed, counts, num_iters, num_samples, lists=True):
    """The draws of a gfw_pose_almeida call on the host (gfw_pose_draws; no context, no GPU): ``counts`` = the points of each pair ->
    (triples int32 [n_pairs][num_iters][3], one int32 sample list [num_iters][min(n, num_samples)] per pair, or None without ``lists``).
    One valid draw per seed from a counter-based generator: not rand's sequence."""
    n = len(counts)
    first = np.zeros(n + 1, dtype=np.int32)
    lens = [min(int(c), int(num_samples)) for c in counts]
    sf = np.zeros(n + 1, dtype=np.int32)
    if n:
        first[1:] = np.cumsum([int(c) for c in counts])
        sf[1:] = np.cumsum([int(num_iters) * m for m in lens])
    triples = np.zeros((n, int(num_iters), 3), dtype=np.int32)
    flat = np.zeros(max(int(sf[-1]), 1), dtype=np.int32)
    lib = abi.load_library()
    rc = lib.gfw_pose_draws(int(seed) & (2 ** 64 - 1), first.ctypes.data, n, int(num_iters), int(num_samples), triples.ctypes.data if triples.size else None,
                            sf.ctypes.data if lists else None, flat.ctypes.data if lists else None)
    if rc < 0:
        raise GfwError(rc, lib.gfw_last_error().decode())
    if not lists:
        return triples, None
    return triples, [flat[sf[p]:sf[p + 1]].reshape(int(num_iters), lens[p]).copy() for p in range(n)]


def pose_draws_k(seed, counts, num_iters, k=8):
    """k distinct indices a round and pair on the host (gfw_pose_draws_k; no context, no GPU): ``counts`` = the points of each pair -> int32 [n_pairs][num_iters][k]
    (zeros for a pair under k points).  gfw_pose_draws' generator: at k = 3 its triples to the bit.  The octets of ``Backend.pose_essential`` are k = 8."""
    n = len(counts)
    first = np.zeros(n + 1, dtype=np.int32)
    if n:
        first[1:] = np.cumsum([int(c) for c in counts])
    tuples = np.zeros((n, int(num_iters), int(k)), dtype=np.int32)
    lib = abi.load_library()
    rc = lib.gfw_pose_draws_k(int(seed) & (2 ** 64 - 1), first.ctypes.data, n, int(num_iters), int(k), tuples.ctypes.data if tuples.size else None)
    if rc < 0:
        raise GfwError(rc, lib.gfw_last_error().decode())
    return tuples


def lowpass_gyro(freq, sample_rate, xyz, has=None):
    """Lowpass::filter_gyro_forward_backward (filtering.rs:46-74) of a gyro series on the host (gfw_lowpass_gyro; no context, no GPU): -> (float64 [n][3], applied).
    ``has``: None or [n], 0 = `gyro: None` (skipped, the filter state does not advance).  ``applied`` is False — the data returned as given — where the reference's
    Coefficients::from_params fails (2 * freq > sample_rate) and the reference goes on unfiltered."""
    v = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(v)
    h = None if has is None else np.ascontiguousarray((np.asarray(has).reshape(-1) != 0).astype(np.uint8))
    assert h is None or len(h) == len(v)
    lib = abi.load_library()
    rc = lib.gfw_lowpass_gyro(float(freq), float(sample_rate), v.ctypes.data if len(v) else None, h.ctypes.data if h is not None and len(h) else None, len(v))
    if rc < 0:
        raise GfwError(rc, lib.gfw_last_error().decode())
    return v, rc == 0


def zoom_smooth(fov_minimal, adaptive_zoom_window, scaled_fps, method=0, trim_ranges=()):
    """zooming/mod.rs:55-68 + zoom_dynamic.rs on the host (gfw_zoom_smooth; no context, no GPU): -> (fovs, fov_minimal after the trim ranges), float64 [n].
    window < -0.9 static zoom, > 0.0001 dynamic (method 0 Gaussian filter, 1 envelope follower), else 1.0; ``trim_ranges``: (start, end) fractions of the clip."""
    v = np.ascontiguousarray(fov_minimal, dtype=np.float64).reshape(-1)
    tr = np.ascontiguousarray(trim_ranges, dtype=np.float64).reshape(-1, 2)
    out, mn = np.zeros_like(v), np.zeros_like(v)
    lib = abi.load_library()
    rc = lib.gfw_zoom_smooth(v.ctypes.data if len(v) else None, len(v), float(adaptive_zoom_window), float(scaled_fps), int(method),
                             tr.ctypes.data if len(tr) else None, len(tr), out.ctypes.data if len(v) else None, mn.ctypes.data if len(v) else None)
    if rc != 0:
        raise GfwError(rc, lib.gfw_last_error().decode())
    return out, mn


def pack_matrices(matrices):
    """[rows][14] f32 -> libgfwarp's packed [rows][16] layout (host libm trig for the IBIS slots)."""
    m = np.ascontiguousarray(matrices, dtype=np.float32)
    out = np.empty((m.shape[0], 16), dtype=np.float32)
    rc = abi.load_library().gfw_pack_matrices(m.ctypes.data, m.shape[0], out.ctypes.data)
    if rc != 0:
        raise GfwError(rc, abi.load_library().gfw_last_error().decode())
    return out


class FrameCall:
    """Pre-marshalled ``gfw_undistort_frame`` call (the per-frame hot loop of a renderer keeps these around so that
    no ctypes objects are built per frame)."""

    def __init__(self, backend, planes, params, pixel_types, matrices, matrix_count=None):
        n = len(planes)
        self.be, self.n = backend, n
        self.barr = (abi.Buffers * n)(*planes)
        self.parr = (abi.KernelParams * n)(*params)
        self.tarr = (C.c_int * n)(*[abi.PIXEL_TYPES[t][0] if isinstance(t, str) else t for t in pixel_types])
        self.mp, self.mc, self.m = _matrix_arg(matrices, matrix_count)
        self.fn = backend.lib.gfw_undistort_frame

    def __call__(self):
        rc = self.fn(self.be.ctx, self.n, self.barr, self.parr, self.tarr, self.mp, self.mc, None, 0)
        if rc != 0:
            self.be._check(rc)


class PlaneCalls:
    """Pre-marshalled per-plane ``gfw_undistort_image`` calls of ONE frame, plane p through backend p — the call sequence of the reference's render loop
    (one process_pixels per plane, each plane its own Stabilization / backend object, src/rendering/mod.rs:494-545)."""

    def __init__(self, backends, planes, params, matrices, matrix_count=None):
        mp, mc, self.m = _matrix_arg(matrices, matrix_count)
        self.keep = [(abi.Buffers.from_buffer_copy(b), abi.KernelParams.from_buffer_copy(p)) for b, p in zip(planes, params)]
        for i, (_, p) in enumerate(self.keep):
            p.plane_index = i
        self.items = [(be.lib.gfw_undistort_image, be.ctx, C.byref(b), C.byref(p), mp, mc, be) for be, (b, p) in zip(backends, self.keep)]

    def __call__(self):
        for fn, ctx, b, p, mp, mc, be in self.items:
            rc = fn(ctx, b, p, mp, mc, None, 0, None, 0)
            if rc != 0:
                be._check(rc)


class ClipCall:
    """Pre-marshalled ``gfw_undistort_clip`` call: ``frames`` is a list of per-frame plane lists (``Buffers``), ``matrices`` a list
    of per-frame tables (device pointers, or numpy [rows][14] arrays), ``params`` / ``pixel_types`` are shared by all frames."""

    def __init__(self, backend, frames, params, pixel_types, matrices, matrix_count=None):
        nf, n = len(frames), len(frames[0])
        self.be, self.nf, self.n = backend, nf, n
        self.barr = (abi.Buffers * (nf * n))(*[b for fr in frames for b in fr])
        self.parr = (abi.KernelParams * n)(*params)
        self.tarr = (C.c_int * n)(*[abi.PIXEL_TYPES[t][0] if isinstance(t, str) else t for t in pixel_types])
        args = [_matrix_arg(m, matrix_count) for m in matrices]
        self.keep = [a[2] for a in args if a[2] is not None]
        self.marr = (C.c_void_p * nf)(*[a[0] for a in args])
        self.mc = next((a[1] for a in reversed(args) if a[2] is not None), matrix_count)
        self.fn = backend.lib.gfw_undistort_clip

    def __call__(self):
        rc = self.fn(self.be.ctx, self.nf, self.n, self.barr, self.parr, self.tarr, self.marr, self.mc)
        if rc != 0:
            self.be._check(rc)


class ClipParamsCall(ClipCall):
    """Pre-marshalled ``gfw_undistort_clip_params`` call: as ``ClipCall``, but ``params`` is a list of per-frame plane lists (``KernelParams``) — frame f's
    own blocks, as ``FrameTransform::at_timestamp`` fills them per frame (adaptive zoom, keyframes, the render loop's fill flag)."""

    def __init__(self, backend, frames, params, pixel_types, matrices, matrix_count=None):
        if len(params) != len(frames) or any(len(p) != len(fr) for p, fr in zip(params, frames)):
            raise ValueError("params: one list of per-plane KernelParams per frame")
        super().__init__(backend, frames, params[0], pixel_types, matrices, matrix_count)
        self.parr = (abi.KernelParams * (self.nf * self.n))(*[p for fp in params for p in fp])
        self.fn = backend.lib.gfw_undistort_clip_params


class ClipLensCall(ClipParamsCall):
    """Pre-marshalled ``gfw_undistort_clip_lens`` call: as ``ClipParamsCall``, for a clip whose lens (f, c, k, r_limit), refraction coefficient and mesh move
    per frame as well.  ``meshes``: ``None``, or one entry per frame — ``None`` or the frame's ``mesh_correction`` block (f32, at most 839 values)."""

    def __init__(self, backend, frames, params, pixel_types, matrices, matrix_count=None, meshes=None):
        super().__init__(backend, frames, params, pixel_types, matrices, matrix_count)
        self.fn = backend.lib.gfw_undistort_clip_lens
        self.mesh_keep, self.mesh_ptrs, self.mesh_lens = [], None, None
        if meshes is not None:
            if len(meshes) != self.nf:
                raise ValueError("meshes: one entry (or None) per frame")
            ptrs, lens, last = [], [], (None, None)
            for m in meshes:
                if m is None or len(m) == 0:
                    ptrs.append(None); lens.append(0)
                    continue
                if m is not last[0]:                          # (the same object on consecutive frames: one array, one pointer — the library uploads it once)
                    last = (m, np.ascontiguousarray(m, dtype=np.float32))
                    self.mesh_keep.append(last[1])
                ptrs.append(last[1].ctypes.data); lens.append(last[1].size)
            self.mesh_ptrs, self.mesh_lens = (C.c_void_p * self.nf)(*ptrs), (C.c_size_t * self.nf)(*lens)

    def __call__(self):
        rc = self.fn(self.be.ctx, self.nf, self.n, self.barr, self.parr, self.tarr, self.marr, self.mc, self.mesh_ptrs, self.mesh_lens)
        if rc != 0:
            self.be._check(rc)


def run_plane(src, in_size, dst, out_size, params, pixel_type, model, digital, matrices, mesh=None, **rects):
    """Convenience: create a backend, warp one HOST plane in place into ``dst``."""
    b = host_buffers(src, in_size, dst, out_size, **rects)
    be = Backend(params, pixel_type, model, digital, b)
    try:
        be.undistort_image(b, params, matrices, mesh)
    finally:
        be.close()


def run_frame(frame, fused=True, per_plane=False, variant=None, jit=None):
    """Warp every plane of a ``synthetic.SyntheticFrame`` from HOST buffers; returns output copies.

    fused=False forces the generic per-plane kernel (GFW_OPT_KERNEL_VARIANT = 1); per_plane=True issues one
    ``gfw_undistort_image`` per plane, the way the reference's render loop does; jit sets GFW_OPT_JIT (2: the frame waits
    for its run-time specialised kernel)."""
    outs = [pl["dst"].copy() for pl in frame.planes]
    bufs = [host_buffers(pl["src"], pl["size"], o, pl["out_size"]) for pl, o in zip(frame.planes, outs)]
    params = [pl["params"] for pl in frame.planes]
    types = [pl["pixel_type"] for pl in frame.planes]
    if per_plane:
        for b, p, t in zip(bufs, params, types):
            be = Backend(p, t, frame.model, frame.digital, b)
            try:
                if not fused:
                    be.set_option(abi.OPT_KERNEL_VARIANT, 1)
                be.undistort_image(b, p, frame.matrices)
            finally:
                be.close()
        return outs
    be = Backend(params[0], types[0], frame.model, frame.digital, bufs[0])
    try:
        if not fused:
            be.set_option(abi.OPT_KERNEL_VARIANT, 1)
        elif variant is not None:
            be.set_option(abi.OPT_KERNEL_VARIANT, variant)
        if jit is not None:
            be.set_option(abi.OPT_JIT, jit)
        be.undistort_frame(bufs, params, types, frame.matrices)
    finally:
        be.close()
    return outs
