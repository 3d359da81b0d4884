"""gyroflow::find_offsets_essential / initial_offset_fast (include/gfwarp.hpp: the gyro-match offset search over gfw_sync_gyro_search) driven by a C++ program
(tests/cpp/test_sync_gyro.cpp) against a dump of the numpy statement's results (tests/_syncgyrostmt.py) for two planted clips.  CPU: the guards, the loud failure
without a context, the median rule, and the host half — range cut, gyro window, max-angle skip, low-pass — equal to the statement's staged ranges to the bit.
GPU: the offsets and the fast initial offset equal the statement's to the bit."""
import os
import subprocess

import pytest

import _syncgyrostmt as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")

# (fps, gyro Hz, planted ms, search_size): short clips — the dump holds every sample; 30 fps takes the unfiltered path, a None in either series
CLIPS = [(60.0, 500.0, 41.7, 300.0), (30.0, 400.0, -88.2, 250.0)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_sync_gyro")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sync_gyro.cpp"), "-o", out,
                           "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def h(v):
    return float(v).hex()


def dump(path, k):
    """the clip, the statement's staged ranges, its offsets and its fast initial offset, as text"""
    fps, rate, offs, size = CLIPS[k]
    c = G.Clip(fps, rate, offs, seed=300 + k, duration_s=6.0, span=[(1.5, 2.5), (3.0, 4.0), (2.0, 2.0), (4.2, 4.7)])
    keys = sorted(c.estimated_gyro)
    c.estimated_gyro[keys[100]] = (c.estimated_gyro[keys[100]][0], None)                              # `gyro: None` on either side
    c.raw_imu[700] = (c.raw_imu[700][0], None)
    for key in keys[int(4.2 * fps):]:                                                                # the last range does not move: skipped by the max-angle rule
        t, g = c.estimated_gyro[key]
        c.estimated_gyro[key] = (t, (g[0] * 0.01, g[1] * 0.01, g[2] * 0.01))
    imu = lambda t, g: "%s %d %s %s %s" % ((h(t), 0, h(0.0), h(0.0), h(0.0)) if g is None else (h(t), 1, h(g[0]), h(g[1]), h(g[2])))
    ins = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, size)
    offsets = G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, size)
    fast = G.initial_offset_fast(offsets, 0.0, size)
    lines = ["%s %s %s %s" % (h(c.duration_ms), h(c.fps), h(0.0), h(size)), str(len(c.estimated_gyro))]
    lines += ["%d %s" % (key, imu(*c.estimated_gyro[key])) for key in sorted(c.estimated_gyro)]
    lines += [str(len(c.raw_imu))] + [imu(t, g) for t, g in c.raw_imu]
    lines += [str(len(c.ranges))] + ["%d %d" % r for r in c.ranges]
    lines.append(str(len(ins)))
    for r in ins:
        lines.append(str(r["index"]))
        for rows, has in ((r["est"], r["est_has"]), (r["gyro"], r["gyro_has"])):
            lines.append(str(len(rows)))
            lines += ["%s %s %s %s %d" % (h(a[0]), h(a[1]), h(a[2]), h(a[3]), 1 if b else 0) for a, b in zip(rows, has)]
    lines += [str(len(offsets))] + ["%s %s %s" % (h(a), h(b), h(cst)) for a, b, cst in offsets]
    lines.append("%s %s" % (h(fast[0]), h(fast[1])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return c, ins, offsets


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("sync_gyro")
    out = []
    for k in range(len(CLIPS)):
        path = str(d / ("clip%d.txt" % k))
        c, ins, offsets = dump(path, k)
        assert [r["index"] for r in ins] == [0, 1] and len(offsets) == 2                              # the empty range and the still one do not reach the search
        for _, value, _ in offsets:
            assert abs(value - c.offset_ms) <= 1.0 + 1000.0 / c.rate
        out.append(path)
    return out


@pytest.mark.parametrize("k", range(len(CLIPS)))
def test_cpp_find_offsets_essential_host_half(exe, dumps, k):
    out = subprocess.run([exe, "validate", dumps[k]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok: 2 of 4 ranges" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CLIPS)))
def test_cpp_find_offsets_essential_on_the_device(exe, dumps, k):
    out = subprocess.run([exe, "search", dumps[k]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "search ok: 2 offsets" in out.stdout
