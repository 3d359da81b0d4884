"""gyroflow::find_offsets_rssync (include/gfwarp.hpp: the rs-sync adapter over gfw_sync_rs_search) driven by a C++ program (tests/cpp/test_rs_sync.cpp) against the
numpy statement's stored results, tests/golden/rs_sync_cpp.txt (`PYTHONPATH=. python tests/test_cpp_rs_sync.py` rewrites it; a CPU test holds the stored results to the
statement run on the stored inputs).  Two runs over the same planted clip (200 Hz track, 6 pairs of 24 points, truth 7.3 ms): one search that accepts both of its ranges, one started 40 ms
off whose picks the 90 % rule refuses.  CPU: ranges that reach no search, the loud failure without a context.  GPU: timestamps, offsets and costs to the bit."""
import os
import subprocess

import numpy as np
import pytest

import _posesscase as EC
import _posessstmt as ES
import _rssynccase as RC
import _rssyncstmt as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gyroflow_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "rs_sync_cpp.txt")
RUNS = [(0.0, 30.0), (40.0, 30.0)]                                                   # (initial_offset, search_size) ms


def h(v):
    return float(v).hex()


def stated():
    """the clip, its ranges and what the adapter's rules make of the statement's search for every run"""
    cam = ES.Camera(EC.pinhole_clip(), RC.FLOW)
    cfg = RS.Cfg(readout_ms=12.0)
    track = RC.track(200.0, seconds=2.0)
    pairs = RC.plant_range(cam, [24] * 6, 0.0073, 12.0, RC.unit((1.0, 0.4, 0.2), 0.5), 21)
    ranges = [(pairs[0][0], pairs[3][0] + 1), (7, 7), (pairs[2][0], pairs[5][0] + 1), (pairs[5][0], pairs[5][0] + 1)]      # 4 pairs; empty; 4 pairs; one pair (skipped)
    runs = runs_of(cam, cfg, track, pairs, ranges)
    return cam, cfg, track, pairs, ranges, runs


def fixture_text():
    cam, cfg, track, pairs, ranges, runs = stated()
    c = RC.cfg_of(cam, cfg)
    lines = [bytes(cam.kp).hex(), "%d %d" % (cam.clip.model, cam.clip.digital),
             "%d %d %d %d %d %d %d %d %d %s %s %s %s" % (c.video_width, c.video_height, c.flow_width, c.flow_height, c.rounds, c.refine, c.hypotheses, c.refits, c.jacobi_sweeps,
                                                         h(c.frame_readout_time_ms), h(c.step_s), h(c.loss_scale), " ".join(h(c.camera_matrix[i]) for i in range(9))),
             str(len(track[0]))]
    lines += ["%d %s" % (t, " ".join(h(v) for v in q)) for t, q in zip(track[0], track[1])]
    lines += [str(len(ranges))] + ["%d %d" % r for r in ranges] + [str(len(pairs))]
    for ta, tb, a, b in pairs:
        lines.append("%d %d %d" % (ta, tb, len(a)))
        lines += ["%s %s %s %s" % (h(x[0]), h(x[1]), h(y[0]), h(y[1])) for x, y in zip(a, b)]
    lines.append(str(len(runs)))
    for initial_offset, search_size, out in runs:
        lines.append("%s %s %d" % (h(initial_offset), h(search_size), len(out)))
        lines += ["%s %s %s" % (h(t), h(o), h(c_)) for t, o, c_ in out]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgfwarp.so")), "libgfwarp.so not built"
    out = str(tmp_path_factory.mktemp("cpp") / "test_rs_sync")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_rs_sync.cpp"), "-o", out, "-L" + LIBDIR, "-lgfwarp", "-ldl", "-Wl,-rpath," + LIBDIR])
    return out


def runs_of(cam, cfg, track, pairs, ranges):
    """what the adapter's rules make of the statement's search for every run of RUNS"""
    live = [[p for p in pairs if a <= p[0] < b] for a, b in ranges]
    live = [l for l in live if len(l) >= 2]
    runs = []
    for initial_offset, search_size in RUNS:
        initial_delay = -initial_offset
        res = RS.search(cam, cfg, track[0], track[1], live, initial_delay / 1000.0, search_size / 1000.0)[0]
        out = []
        for l, r in zip(live, res):
            offset = r[4] * 1000.0
            if r[0] and abs(offset - initial_delay) < search_size * 0.9:
                out.append((float(l[0][0] + l[-1][1]) / 2.0 / 1000.0, -offset - (cfg.readout_ms / 1000.0 * 1000.0 / 2.0), r[5]))
        runs.append((initial_offset, search_size, out))
    return runs


def stored():
    """the fixture's own track, ranges, pairs and runs, read back"""
    with open(FIXTURE) as f:
        tok = f.read().split()[1 + 2 + 9 + 3 + 9:]                                    # behind the KernelParams, the lens ids and the configuration (9 integers, 3 reals, K)
    at = [0]

    def take(n=1):
        at[0] += n
        return tok[at[0] - n:at[0]]
    n = int(take()[0])
    rows = [take(5) for _ in range(n)]
    track = (np.array([int(r[0]) for r in rows], dtype=np.int64), np.array([[float.fromhex(v) for v in r[1:]] for r in rows]))
    ranges = [tuple(int(v) for v in take(2)) for _ in range(int(take()[0]))]
    pairs = []
    for _ in range(int(take()[0])):
        ta, tb, k = (int(v) for v in take(3))
        pts = np.array([[float.fromhex(v) for v in take(4)] for _ in range(k)], dtype=np.float32)
        pairs.append((ta, tb, pts[:, :2].copy(), pts[:, 2:].copy()))
    runs = []
    for _ in range(int(take()[0])):
        io, ss, k = take(3)
        runs.append((float.fromhex(io), float.fromhex(ss), [tuple(float.fromhex(v) for v in take(3)) for _ in range(int(k))]))
    assert at[0] == len(tok)
    return track, ranges, pairs, runs


def test_the_stored_fixture_is_the_statements():
    """the stored results are what the statement makes of the stored inputs (+ - * / sqrt and the lens inverse only: the plant's sines are not run again); the first
    run accepts both ranges within a gyro sample period of the truth, the second is refused"""
    track, ranges, pairs, runs = stored()
    cam, cfg = ES.Camera(EC.pinhole_clip(), RC.FLOW), RS.Cfg(readout_ms=12.0)
    with open(FIXTURE) as f:
        assert f.read().split()[0] == bytes(cam.kp).hex()
    assert runs_of(cam, cfg, track, pairs, ranges) == runs
    assert [len(r[2]) for r in runs] == [2, 0] and [r[:2] for r in runs] == RUNS
    for _, offset, _ in runs[0][2]:
        assert abs(offset - (-7.3 - 6.0)) < 5.0
    assert os.path.getsize(FIXTURE) < 128 * 1024


def test_cpp_rs_sync_host_half(exe):
    out = subprocess.run([exe, "validate", FIXTURE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "validate ok: 4 ranges, 6 pairs, 2 runs" in out.stdout


@pytest.mark.gpu
def test_cpp_find_offsets_rssync_on_the_device(exe):
    out = subprocess.run([exe, "search", FIXTURE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "search ok: 2 runs, 2 offsets" in out.stdout


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(fixture_text())
    print("wrote", FIXTURE)
