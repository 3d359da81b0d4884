"""Float64 host statement of FrameTransform::at_timestamp's matrix loop (frame_transform.rs:221-308) — the checker of the
device-side matrix builder (gfw_build_matrices*).  Test infrastructure: written from the cited Rust, independent of the device
code; not part of the product package.

  quat_at / offset_at      gyro_source/mod.rs:857-908 (sync offsets subtracted per lookup, identity when duration <= 0)
  catmull_rom_at           gyro_source/splines.rs:22-84
  row_matrices_from_tracks frame_transform.rs:221-308 incl. IBIS/OIS terms (:234-241, :270-289) and suppress_rotation (:291-296)
"""
import math

import numpy as np

from gyroflow_amd.synthetic import quat_mul, quat_to_matrix


def slerp(a, b, t):
    """nalgebra UnitQuaternion::slerp (shorter arc)."""
    c = float(np.dot(a, b))
    if c < 0.0:
        b, c = -b, -c
    if abs(c) >= 1.0:
        return a.copy()
    hang = math.acos(c)
    s = math.sqrt(1.0 - c * c)
    if s == 0.0:
        return a.copy()
    return a * (math.sin((1.0 - t) * hang) / s) + b * (math.sin(t * hang) / s)


def _as_i64(v):
    """Rust `f64 as i64`: truncate toward zero, saturating, NaN -> 0 (total: infinities and values beyond i64 included)."""
    if v != v:
        return 0
    if v >= 9223372036854775807.0:
        return 2 ** 63 - 1
    if v <= -9223372036854775808.0:
        return -2 ** 63
    return int(math.trunc(v))


def _round(v):
    """f64::round: to the nearest integer, halves away from zero, exactly (no `v + 0.5`, which rounds); NaN and the infinities pass through."""
    if v != v or math.isinf(v):
        return v
    t = float(math.trunc(v))
    return t + math.copysign(1.0, v) if abs(v - t) >= 0.5 else t


def offset_at(offsets, timestamp_ms):
    """GyroSource::offset_at_timestamp (gyro_source/mod.rs:884-908); offsets = (ts_us ascending, offsets_ms) or None."""
    if offsets is None or len(offsets[0]) == 0:
        return 0.0
    ts, v = offsets
    if len(ts) == 1:
        return float(v[0])
    timestamp_us = _as_i64(timestamp_ms * 1000.0)
    lookup = max(min(timestamp_us, int(ts[-1]) - 1), int(ts[0]) + 1)
    i = int(np.searchsorted(ts, lookup, side="right")) - 1
    if i < 0:
        return 0.0
    if int(ts[i]) == lookup:
        return float(v[i])
    if i + 1 >= len(ts):
        return 0.0
    fract = float(timestamp_us - int(ts[i])) / float(int(ts[i + 1]) - int(ts[i]))
    return float(v[i]) + (float(v[i + 1]) - float(v[i])) * fract


def quat_at(ts_us, quats, timestamp_ms, offsets=None, duration_ms=1.0):
    """GyroSource::quat_at_timestamp (gyro_source/mod.rs:857-882)."""
    if len(ts_us) < 2 or not (duration_ms > 0.0):
        return np.array([1.0, 0.0, 0.0, 0.0])
    timestamp_ms = timestamp_ms - offset_at(offsets, timestamp_ms)
    lookup = max(min(_as_i64(_round(timestamp_ms * 1000.0)), int(ts_us[-1])), int(ts_us[0]))      # ((x * 1000.0).round() as i64).min(last).max(first)
    i = int(np.searchsorted(ts_us, lookup, side="right")) - 1
    if ts_us[i] == lookup or i + 1 >= len(ts_us):
        return quats[i].copy()
    fract = float(lookup - ts_us[i]) / float(ts_us[i + 1] - ts_us[i])
    return slerp(quats[i], quats[i + 1], fract)


def catmull_rom_at(points, t):
    """CatmullRom<Vector3<f64>>::interpolate (splines.rs:22-84); points = [n][4] (position, x, y, z); None when outside."""
    n = len(points)
    if n < 2 or t != t:
        return None
    pos = [float(p[0]) for p in points]
    lo = int(np.searchsorted(pos, t, side="left"))
    if lo < n and pos[lo] == t:
        if lo == n - 1:
            return None
        lower = lo
    else:
        if lo >= n or lo == 0:
            return None
        lower = lo - 1
    if lower + 1 >= n:
        return None
    a = np.asarray(points[lower][1:4], dtype=np.float64)
    b = np.asarray(points[lower + 1][1:4], dtype=np.float64)
    k = (t - pos[lower]) / (pos[lower + 1] - pos[lower])
    x = a * 2.0 - b if lower <= 0 else np.asarray(points[lower - 1][1:4], dtype=np.float64)
    y = b * 2.0 - a if lower + 2 >= n else np.asarray(points[lower + 2][1:4], dtype=np.float64)
    return ((((a * 3.0 - x) - b * 3.0) + y) * 0.5) * k * k * k + ((b - x) * 0.5) * k + a + (((b * 4.0 + a * -5.0 + x + x) - y) * 0.5) * k * k


def row_matrices_from_tracks(org, smoothed, nk, timestamp_ms, frame_readout_time_ms, rows, readout_dim,
                             video_rotation_deg=0.0, framebuffer_inverted=False, per_frame_offset_ms=0.0,
                             offsets=None, duration_ms=1.0, suppress_rotation=0, stab=None):
    """Float64 host statement of frame_transform.rs:221-308 over sampled tracks; returns [rows][14] f32.

    stab: None or dict(offset, sensor_size, crop_area, pixel_pitch, width, height, ibis=[n][4], ois=[n][4])."""
    ts = timestamp_ms + per_frame_offset_ms
    start_ts = ts - frame_readout_time_ms / 2.0
    row_t = frame_readout_time_ms / readout_dim
    q1 = quat_at(org[0], org[1], ts, offsets, duration_ms)
    q1 = np.array([q1[0], -q1[1], -q1[2], -q1[3]]) / np.dot(q1, q1)
    sm = quat_at(smoothed[0], smoothed[1], ts, offsets, duration_ms)
    a = math.radians(video_rotation_deg)
    rot = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    out = np.zeros((rows, 14), dtype=np.float32)
    inv = -1.0 if framebuffer_inverted else 1.0
    for y in range(rows):
        qt = start_ts + row_t * y if abs(frame_readout_time_ms) > 0.0 else start_ts
        q = quat_mul(sm, quat_mul(q1, quat_at(org[0], org[1], qt, offsets, duration_ms)))
        r = rot @ quat_to_matrix(q)
        if framebuffer_inverted:
            r[0, 2] *= -1.0; r[1, 2] *= -1.0; r[2, 0] *= -1.0; r[2, 1] *= -1.0
        else:
            r[0, 1] *= -1.0; r[0, 2] *= -1.0; r[1, 0] *= -1.0; r[2, 0] *= -1.0
        terms = np.zeros(5, dtype=np.float32)
        if stab is not None:
            scale_x = stab["width"] / stab["crop_area"][2] / stab["pixel_pitch"][0]
            scale_y = stab["height"] / stab["crop_area"][3] / stab["pixel_pitch"][1] * inv
            c1, c3 = stab["crop_area"][1], stab["crop_area"][3]
            y_sensor = (float(y) - 0.0) * ((c1 + c3) - c1) / (stab["height"] - 0.0) + c1
            if framebuffer_inverted:
                y_sensor = stab["sensor_size"][1] - y_sensor
            s = catmull_rom_at(stab["ibis"], y_sensor + stab["offset"])
            o = catmull_rom_at(stab["ois"], y_sensor + stab["offset"])
            s = np.zeros(3) if s is None else s
            o = np.zeros(3) if o is None else o
            ra = s[2] / 1000.0 * inv
            terms = np.array([s[0] * scale_x, s[1] * scale_y, ra * (math.pi / 180.0), o[0] * scale_x, o[1] * scale_y]).astype(np.float32)
        if suppress_rotation:
            r = np.eye(3)
            if suppress_rotation == 2:
                terms[:] = 0.0
        out[y, :9] = np.linalg.pinv(nk @ r, rcond=1e-6).reshape(9).astype(np.float32)
        out[y, 9:14] = terms
    return out
